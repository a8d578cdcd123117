"""The data-parallel path on the real device: one RCCL rank with the reducer forced on, so bucket events, the side
stream, the NCCL(=RCCL) all-reduce calls and the join before the fused optimiser all execute on the MI355X.
(Multi-rank semantics are covered on CPU/gloo by tests/test_dist_cpu.py; the 8-GPU run is the driver's.)"""
import os
import socket

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_trainer_step_through_rccl_reducer(monkeypatch):
    from oracle import fill
    from pytorch_segmentation_amd.models import DeepLabV3Plus
    from pytorch_segmentation_amd.utils import Trainer, compute_loss
    monkeypatch.setenv('MASTER_ADDR', '127.0.0.1')
    monkeypatch.setenv('MASTER_PORT', str(_free_port()))
    monkeypatch.setenv('PSEG_FORCE_REDUCER', '1')
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        x = fill.images('distgpu/x', (4, 3, 64, 64)).cuda()
        t = fill.labels('distgpu/t', (4, 64, 64), 21, block=8).cuda()

        def run(force, graph=False, native=False):
            os.environ['PSEG_FORCE_REDUCER'] = '1' if force else '0'
            os.environ['PSEG_NATIVE_ALLREDUCE'] = '1' if native else '0'
            torch.manual_seed(0)
            m = DeepLabV3Plus(21)
            fill.fill_module_(m, 'distgpu')
            tr = Trainer(m, None, loss_fn=compute_loss, accumulate=2, lr=1e-2, bucket_bytes=8 << 20, graph=graph)
            assert tr.reducer.enabled == force and (tr.reducer.native is not None) == (force and native)
            m.train()
            # two (eager) / four (graph: the first window of a shape runs eagerly, the second captures) optimiser steps of
            # two micro-batches each
            losses = [tr.train_batch(x, t).item() for _ in range(8 if graph else 4)]
            torch.cuda.synchronize()
            return losses, tr.arena.params.clone(), len(tr.reducer.buckets), tr

        l1, p1, nb, _ = run(True)
        l0, p0, _, _ = run(False)
        assert nb >= 10                       # 157 MB of gradients in 8 MiB buckets
        assert l1 == l0                       # one rank: the all-reduce is the identity -> bit-identical training
        assert torch.equal(p1, p0)
        assert l1[2] < l1[0]                  # and it actually trains
        # captured + replayed micro-steps: every bucket's all-reduce hangs behind a MARKER of the replay (lane executor,
        # csrc/lanes.hip) on the side stream -- overlapped with the replayed backward, not trailing it
        lg, pg, _, trg = run(True, graph=True)
        l0g, p0g, _, _ = run(False, graph=True)
        sgs = [sg for sg in trg._graphs.values() if sg is not None]
        assert sgs and all(sg.lanes and sg.lane_info['markers'] >= nb for sg in sgs), [sg.lane_info for sg in sgs]
        assert all(len(sg.marked) == nb for sg in sgs)
        assert lg == l0g and torch.equal(pg, p0g)
        assert lg[:4] == l0[:4]               # and the replayed run is the eager run
        # the library's own RCCL binding (pseg_allreduce_bucket on a communicator built from a unique id that travels through
        # torch.distributed): eager and replayed
        ln, pn, _, trn = run(True, native=True)
        assert ln == l0 and torch.equal(pn, p0)
        lng, png, _, trng = run(True, graph=True, native=True)
        assert lng == l0g and torch.equal(png, p0g)
        trn.reducer.native.close(), trng.reducer.native.close()
        # HRNet: the captured step forks its resolution branches onto lanes of their own (ops.Branches), so a bucket's
        # gradients are spread over several streams when its last gradient kernel is enqueued -- the marker is set where the
        # lanes have been joined (ops.after_branches).  Every bucket marked, replay == eager without a reducer.
        from pytorch_segmentation_amd.models import HRNet

        def run_hr(force, graph):
            os.environ['PSEG_FORCE_REDUCER'] = '1' if force else '0'
            os.environ['PSEG_NATIVE_ALLREDUCE'] = '0'
            torch.manual_seed(0)
            m = HRNet(21)
            fill.fill_module_(m, 'distgpu/hr')
            tr = Trainer(m, None, loss_fn=compute_loss, lr=1e-2, bucket_bytes=4 << 20, graph=graph)
            m.train()
            losses = [tr.train_batch(x, t).item() for _ in range(5)]
            torch.cuda.synchronize()
            return losses, tr.arena.params.clone(), tr

        lh0, ph0, _ = run_hr(False, False)
        lh1, ph1, trh = run_hr(True, True)
        (sgh,) = [sg for sg in trh._graphs.values() if sg is not None]
        nbh = len(trh.reducer.buckets)
        assert nbh >= 4 and sgh.lane_info['lanes'] >= 3 and len(sgh.marked) == nbh, (nbh, sgh.lane_info, len(sgh.marked))
        assert lh1 == lh0 and torch.equal(ph1, ph0)
        # the exchange as reduce-scatter + all-gather (PSEG_EXCHANGE=rs_ag), through torch.distributed and through the
        # library's own binding: still the identity on one rank, bit-identical training
        os.environ['PSEG_EXCHANGE'] = 'rs_ag'
        lr, pr, _, trr = run(True)
        assert trr.reducer.exchange == 'rs_ag' and lr == l0 and torch.equal(pr, p0)
        lrn, prn, _, trrn = run(True, native=True)
        assert lrn == l0 and torch.equal(prn, p0)
        trrn.close()
        assert trrn.reducer.native is None
    finally:
        os.environ.pop('PSEG_EXCHANGE', None)
        os.environ.pop('PSEG_NATIVE_ALLREDUCE', None)
        dist.destroy_process_group()


def test_allreduce_bucket_c_abi_one_rank():
    """include/pseg_amd.h: pseg_comm_unique_id / pseg_comm_init / pseg_allreduce_bucket / pseg_comm_destroy called directly
    (no torch.distributed): a one-rank communicator, an in-place sum over 3 M floats on a side stream = the identity."""
    import ctypes
    from pytorch_segmentation_amd import _lib
    lib = _lib.load()
    assert lib.pseg_comm_available() == 1
    torch.cuda.set_device(0)
    ident = (ctypes.c_char * 128)()
    _lib.call('pseg_comm_unique_id', ctypes.addressof(ident))
    assert any(b != 0 for b in ident.raw)
    h = ctypes.c_int64(0)
    _lib.call('pseg_comm_init', ctypes.addressof(ident), 1, 0, ctypes.byref(h))
    assert h.value != 0
    g = torch.randn(3 << 20, device='cuda')
    want = g.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    _lib.call('pseg_allreduce_bucket', h.value, g.data_ptr(), g.numel(), side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(g, want)
    with pytest.raises(_lib.PsegError):
        _lib.call('pseg_allreduce_bucket', 0, g.data_ptr(), g.numel(), side.cuda_stream)
    # the same sum as a reduce-scatter + all-gather pair (PSEG_EXCHANGE=rs_ag): one rank owns the whole bucket
    _lib.call('pseg_reduce_scatter_bucket', h.value, g.data_ptr(), g.numel(), 0, side.cuda_stream)
    _lib.call('pseg_all_gather_bucket', h.value, g.data_ptr(), g.numel(), 0, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(g, want)
    ver = ctypes.c_int(0)
    _lib.call('pseg_comm_version', ctypes.byref(ver))
    assert ver.value >= 20000          # RCCL reports an NCCL-compatible version code (2.x.y -> 2xxyy)
    with pytest.raises(_lib.PsegError):
        _lib.call('pseg_reduce_scatter_bucket', 0, g.data_ptr(), g.numel(), 0, side.cuda_stream)
    _lib.call('pseg_comm_destroy', h.value)


def test_bench_two_rank_rehearsal():
    """bench.py under the driver's N>1 launch line (torch.distributed.run, two ranks) -- both ranks on the one GPU of the
    test box, gradients over gloo (PSEG_BENCH_REHEARSAL=1).  Not a measurement: it proves that the launch contract, the
    barriers, the max-over-ranks timing and the metered extra step (a full training step with its bucketed all-reduce,
    which EVERY rank has to take part in) run to completion and that rank 0 prints exactly one JSON line."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSEG_BENCH_REHEARSAL='1', PSEG_EXCHANGE='rs_ag')
    env.pop('PSEG_FORCE_REDUCER', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), os.path.join(repo, 'bench.py'), '--full', '--gpus', '2', '--steps', '2',
           '--warmup', '1', '--batch', '2', '--size', '128']
    r = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 2 and out['steps'] == 2 and out['value'] > 0
    assert out['config']['global_batch'] == 4 and out['scaling'] == 'weak'
    assert out['roofline'] is not None and out['cpu_baseline'] is None
    # the N>1 line explains itself: who took part, what was exchanged how, and what the exchange cost beyond backward
    mg = out['multi_gpu']
    assert mg['ranks_seen'] == 2 and mg['distinct_devices'] == 1 and len(mg['devices']) == 2      # (rehearsal: one GPU)
    assert mg['exchange']['mode'] == 'rs_ag' and mg['exchange']['buckets'] >= 4 and mg['exchange']['world'] == 2
    assert abs(mg['exchange']['bytes'] - 156.6e6) < 2e6
    assert mg['step_nocomm_ms'] > 0 and mg['exposed_comm_ms'] == mg['exposed_comm_ms']


def test_bench_four_rank_rehearsal():
    """the same launch line with FOUR ranks (all on the test box's one GPU, gradients over gloo) at
    128x128, batch 2 per rank: four processes through init, warm-up, the barrier-bracketed timed steps, the max-over-ranks
    reduction, the collectives-skipped re-timing, the re-broadcast of rank 0's model and the metered step -- one JSON line whose
    `multi_gpu` object names four ranks, the exchange that ran and what it cost.  Control flow only; no curve exists."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PSEG_BENCH_REHEARSAL='1', PSEG_EXCHANGE='allreduce')
    env.pop('PSEG_FORCE_REDUCER', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '4', '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), os.path.join(repo, 'bench.py'), '--full', '--gpus', '4', '--steps', '2',
           '--warmup', '1', '--batch', '2', '--size', '128']
    r = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['n_gpus'] == 4 and out['steps'] == 2 and out['value'] > 0
    assert out['config']['global_batch'] == 8 and out['config']['parallelism'] == 'dp4' and out['scaling'] == 'weak'
    assert out['roofline'] is not None and out['roofline']['whole_step']['frac'] > 0 and out['cpu_baseline'] is None
    mg = out['multi_gpu']
    assert mg['ranks_seen'] == 4 and mg['distinct_devices'] == 1 and sorted(d['rank'] for d in mg['devices']) == [0, 1, 2, 3]
    assert mg['exchange']['mode'] == 'allreduce' and mg['exchange']['buckets'] >= 4 and mg['exchange']['world'] == 4
    assert abs(mg['exchange']['bytes'] - 156.6e6) < 2e6
    assert mg['step_nocomm_ms'] > 0 and mg['exposed_comm_ms'] == mg['exposed_comm_ms']


# ---------------------------------------------------------------------------------------------------------------------
# Two-rank gradient parity of the REAL models (reference train.py:33-35,112-117): two processes share the
# test box's one GPU and exchange gradients over gloo -- the reducer, its buckets, events and side stream, the auxiliary
# weight-gradient stream and the fused optimiser are the production code; only the transport differs from RCCL.
_DP_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ['PSEG_REPO'])
from oracle import fill
from pytorch_segmentation_amd import models
from pytorch_segmentation_amd.utils import Trainer, compute_loss
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
name, out = sys.argv[1], sys.argv[2]
use_graph = len(sys.argv) > 3 and sys.argv[3] == 'graph'
torch.cuda.set_device(0)
dist.init_process_group('gloo', init_method='env://', world_size=world, rank=rank)
cls, nc, S = {'deeplabv3plus': (models.DeepLabV3Plus, 21, 128), 'unet': (models.UNet, 2, 128)}[name]
torch.manual_seed(100 + rank)                 # every rank starts from DIFFERENT random weights and BN buffers ...
m = cls(nc)
with torch.no_grad():
    for b in m.buffers():
        if b.is_floating_point():
            b.add_(0.01 * rank)
if rank == 0:
    fill.fill_module_(m, 'dp/' + name)        # ... rank 0 holds the model the run is about
tr = Trainer(m, None, loss_fn=compute_loss, accumulate=2, lr=1e-3, bucket_bytes=8 << 20, graph=use_graph)
assert tr.reducer.enabled and tr.reducer.world == world
if os.environ.get('PSEG_NATIVE_ALLREDUCE') == '1':
    # the library's own binding (csrc/comm.hip) over the library PSEG_RCCL_PATH names: here the two-rank stand-in
    d = tr.reducer.describe()
    assert tr.reducer.native is not None and d['native'] and d['mode'] == os.environ.get('PSEG_EXCHANGE', 'allreduce'), d
    assert d.get('rccl_version') == 99900, d          # (the stand-in's marker version: really bound, not torch's librccl)
    # bucket sizes that are no multiple of the world size exercise the remainder all-reduce of rs_ag
    print('[dp worker %d] exchange %s' % (rank, d), flush=True)
start = tr.arena.params.clone()
m.train()
grads = []
for step in range(4 if use_graph else 3):
    for micro in range(2):
        # global batch of a micro-step = 8 images; rank r takes images [4r, 4r+4)  (DistributedSampler's role)
        x = fill.images('dp/x%d_%d' % (step, micro), (4 * world, 3, S, S))[4 * rank:4 * rank + 4].cuda()
        t = fill.labels('dp/t%d_%d' % (step, micro), (4 * world, S, S), nc, block=8)[4 * rank:4 * rank + 4].cuda()
        if micro == 1:
            # the window's last micro-batch: train_batch all-reduces and steps; grab the reduced arena first
            orig = tr.optimizer.step
            def grab(grad_scale=1.0, mp_state=None, _orig=orig):
                grads.append((tr.arena.grads * grad_scale).cpu().clone())
                _orig(grad_scale=grad_scale, mp_state=mp_state)
            tr.optimizer.step = grab
        tr.train_batch(x, t)
        if micro == 1:
            tr.optimizer.step = orig
torch.cuda.synchronize()
if use_graph:      # the replayed steps exchanged their buckets behind the replay's markers (csrc/lanes.hip)
    sgs = [sg for sg in tr._graphs.values() if sg is not None]
    assert sgs and all(sg.lanes and len(sg.marked) == len(tr.reducer.buckets) for sg in sgs), [sg.lane_info for sg in sgs]
torch.save({'start': start.cpu(), 'params': tr.arena.params.cpu(), 'grads': grads,
            'buffers': {k: v.cpu() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}},
           '%s.rank%d.pt' % (out, rank))
dist.barrier()
dist.destroy_process_group()
'''


@pytest.fixture(scope='module')
def standin_rccl(tmp_path_factory):
    """tests/standin_rccl.cpp built with hipcc: the eight nccl* symbols csrc/comm.hip binds, with N-rank semantics for ranks
    that share ONE device (shared memory + stream-ordered host steps)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    here = os.path.dirname(os.path.abspath(__file__))
    out = tmp_path_factory.mktemp('standin') / 'libstandin_rccl.so'
    subprocess.check_call([hipcc, '-O2', '-shared', '-fPIC', os.path.join(here, 'standin_rccl.cpp'), '-o', str(out), '-lrt'])
    return str(out)


@pytest.mark.parametrize('exchange', ['allreduce', 'rs_ag'])
@pytest.mark.parametrize('name', ['unet', 'unet-graph'])
def test_two_rank_native_exchange_over_standin(tmp_path, standin_rccl, name, exchange):
    """the library's NATIVE exchange (PSEG_NATIVE_ALLREDUCE=1: pseg_comm_init / pseg_allreduce_bucket /
    pseg_reduce_scatter_bucket / pseg_all_gather_bucket, csrc/comm.hip) with TWO ranks.  RCCL refuses two ranks on one device, so
    the library is pointed (PSEG_RCCL_PATH) at tests/standin_rccl.cpp, which gives the eight nccl* symbols N-rank semantics on
    the caller's stream.  One rank cannot falsify any of this: the in-place reduce-scatter / all-gather slice offsets, the
    remainder all-reduce of bucket sizes that are no multiple of the world size, the order of the collectives on the side
    stream behind the bucket events (eager) and behind the replay's markers (unet-graph).  Same assertions as the gloo case:
    reduced gradients equal the single-process run on step 0, parameters bit-identical across ranks after the run."""
    _two_rank_case(tmp_path, name, extra_env={'PSEG_NATIVE_ALLREDUCE': '1', 'PSEG_RCCL_PATH': standin_rccl,
                                               'PSEG_EXCHANGE': exchange})


@pytest.mark.parametrize('exchange', ['allreduce', 'rs_ag'])
@pytest.mark.parametrize('name', ['unet', 'unet-graph'])
def test_four_rank_native_exchange_over_standin(tmp_path, standin_rccl, name, exchange):
    """the same with FOUR ranks sharing the test GPU (the stand-in's host steps have N-rank semantics):
    rank r takes images [4r, 4r+4) of a 16-image micro-batch, rs_ag slices are a quarter of a bucket each and the 8 MiB
    buckets of UNet leave remainders modulo 4 only where a cut does -- the all-gather offsets of ranks 2 and 3 and the
    marker-behind-replay ordering with more than one peer are what two ranks cannot show.  Reduced gradients equal the
    single process that takes the four chunks as accumulation micro-batches; parameters bit-identical on all four ranks."""
    _two_rank_case(tmp_path, name, extra_env={'PSEG_NATIVE_ALLREDUCE': '1', 'PSEG_RCCL_PATH': standin_rccl,
                                               'PSEG_EXCHANGE': exchange}, world=4)


@pytest.mark.parametrize('name', ['deeplabv3plus', 'unet', 'unet-graph'])
def test_two_rank_gradient_parity_real_model(tmp_path, name):
    """N-rank averaged gradients == single-process gradients with BatchNorm applied per rank-sized chunk.
    Two ranks (different seeds!) train DeepLabV3+ / UNet for 3 optimiser steps of 2 micro-batches (accumulate=2,
    weight gradients on the auxiliary stream, 8 MiB buckets -> ~20 all-reduces per step); a single process replays the
    same schedule with every rank's chunk as one more accumulation micro-batch (BN statistics per 4-image chunk, exactly
    what per-replica BatchNorm computes).  Asserted: (1) the initial broadcast made the ranks identical to rank 0's
    model; (2) the reduced, scaled gradient arena of every step matches the single process (the sum is commutative and
    every kernel is deterministic, so the tolerance is fp32 rounding of a different accumulation order: 1e-5);
    (3) parameters are BIT-identical across ranks after 3 steps and match the single process.
    'unet-graph': the same with Trainer(graph=True) on the ranks -- the micro-steps are replayed from captured hipGraphs
    (first sight eager, second captured, then replays) with the collectives issued after the replay."""
    _two_rank_case(tmp_path, name)


def _two_rank_case(tmp_path, name, extra_env=None, world=2):
    import subprocess
    import sys
    from oracle import fill
    from pytorch_segmentation_amd import models
    from pytorch_segmentation_amd.utils import Trainer, compute_loss
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    use_graph = name.endswith('-graph')
    name = name.split('-')[0]
    nsteps = 4 if use_graph else 3
    script = tmp_path / 'dp_worker.py'
    script.write_text(_DP_SCRIPT)
    out = str(tmp_path / 'dp')
    env = dict(os.environ, PSEG_REPO=repo, PSEG_OVERLAP_WGRAD='1')
    env.pop('PSEG_FORCE_REDUCER', None)
    env.update(extra_env or {})
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world), '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), str(script), name, out] + (['graph'] if use_graph else [])
    r = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    ranks = [torch.load('%s.rank%d.pt' % (out, k)) for k in range(world)]
    r0, r1 = ranks[0], ranks[1]
    # single process: same schedule, each rank's chunk as its own accumulation micro-batch
    cls, nc, S = {'deeplabv3plus': (models.DeepLabV3Plus, 21, 128), 'unet': (models.UNet, 2, 128)}[name]
    m = cls(nc)
    fill.fill_module_(m, 'dp/' + name)
    tr = Trainer(m, None, loss_fn=compute_loss, accumulate=2 * world, lr=1e-3)
    assert not tr.reducer.enabled
    start = tr.arena.params.clone()
    assert all(torch.equal(rk['start'], start.cpu()) for rk in ranks)                          # (1)
    m.train()
    single_grads = []
    for step in range(nsteps):
        k = 0
        for micro in range(2):
            for rank in range(world):
                x = fill.images('dp/x%d_%d' % (step, micro), (4 * world, 3, S, S))[4 * rank:4 * rank + 4].cuda()
                t = fill.labels('dp/t%d_%d' % (step, micro), (4 * world, S, S), nc, block=8)[4 * rank:4 * rank + 4].cuda()
                k += 1
                if k == 2 * world:
                    orig = tr.optimizer.step

                    def grab(grad_scale=1.0, mp_state=None, _orig=orig):
                        single_grads.append((tr.arena.grads * grad_scale).cpu().clone())
                        _orig(grad_scale=grad_scale, mp_state=mp_state)
                    tr.optimizer.step = grab
                tr.train_batch(x, t)
                if k == 2 * world:
                    tr.optimizer.step = orig
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()

    for step in range(nsteps):
        assert all(torch.equal(r0['grads'][step], rk['grads'][step]) for rk in ranks[1:])   # every rank holds the same reduced arena
        if step == 0:   # identical parameters on both sides: the same numbers summed in another order
            assert rel(r0['grads'][0], single_grads[0]) < 1e-5                                  # (2)
        # (from step 1 on the two runs' parameters differ in the last bit -- other summation order in step 0 -- and a
        # batch-4 train-mode BatchNorm network at random init amplifies that to 2e-2 .. 8e-1 of the gradient norm within
        # two steps at lr 1e-2: a property of the model, not of the exchange, so only step 0 is
        # compared strictly; later steps get a sanity bound in norm)
        else:
            a, b = r0['grads'][step].double(), single_grads[step].double()
            l2 = ((a - b).norm() / b.norm()).item()
            print('two-rank %s step %d: reduced gradient vs single process, relative L2 %.2e' % (name, step, l2))
            assert l2 < 0.5, (step, l2)
    assert all(torch.equal(r0['params'], rk['params']) for rk in ranks[1:])          # (3)
    assert not torch.equal(r0['params'], start.cpu())
    # per-replica BatchNorm: running statistics are each rank's own (they saw different images)
    k0 = next(k for k in r0['buffers'] if k.endswith('running_mean'))
    assert not torch.equal(r0['buffers'][k0], r1['buffers'][k0])



# ---------------------------------------------------------------------------------------------------------------------
# Distributed evaluation (reference test.py:15-58: every rank evaluates its shard, the per-class counters are summed):
# the replicas' BatchNorm running statistics differ after training (they are per-replica, as under DDP between its
# buffer broadcasts), so test() first gives every rank rank 0's buffers -- DistributedDataParallel's broadcast_buffers.
_EVAL_SCRIPT = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ['PSEG_REPO'])
from oracle import fill
from pytorch_segmentation_amd import models
from pytorch_segmentation_amd.utils import Trainer, compute_loss
import test as test_mod
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
out = sys.argv[1]
torch.cuda.set_device(0)
dist.init_process_group('gloo', init_method='env://', world_size=world, rank=rank)
nc, S = 2, 64
torch.manual_seed(7)
m = models.UNet(nc)
tr = Trainer(m, None, loss_fn=compute_loss, lr=1e-2)
m.train()
for step in range(3):      # train on DIFFERENT data per rank: running statistics drift apart
    x = fill.images('ev/x%d_%d' % (step, rank), (4, 3, S, S)).cuda()
    t = fill.labels('ev/t%d_%d' % (step, rank), (4, S, S), nc, block=8).cuda()
    tr.train_batch(x, t)
before = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}


class DS:
    classes = ['a', 'b']


class Loader:
    dataset = DS()


class Fetch:
    loader = Loader()

    def __init__(self, ranks):
        self.ranks = ranks

    def __iter__(self):
        for r in self.ranks:      # eval shard r: two batches
            for i in range(2):
                yield (fill.images('ev/val%d_%d' % (r, i), (4, 3, S, S)).cuda(),
                       fill.labels('ev/valt%d_%d' % (r, i), (4, S, S), nc, block=8).cuda())


import io, contextlib
buf = io.StringIO()
with contextlib.redirect_stdout(buf):
    miou = test_mod.test(m, Fetch([rank]))
with torch.no_grad():
    logits = m(fill.images('ev/probe', (2, 3, S, S)).cuda()).cpu()
after = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}
single = None
if rank == 0:
    # the same evaluation by ONE process over both shards (no process-group effects: counters are summed locally)
    dist_is = dist.is_initialized
    import pytorch_segmentation_amd.utils.dist as pd
    world_fn = dist.get_world_size
    dist.get_world_size = lambda group=None: 1
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            single = test_mod.test(m, Fetch(list(range(world))))
    finally:
        dist.get_world_size = world_fn
torch.save({'before': before, 'after': after, 'miou': miou, 'single': single, 'logits': logits}, '%s.rank%d.pt' % (out, rank))
dist.barrier()
dist.destroy_process_group()
"""


_MP_SCRIPT = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ['PSEG_REPO'])
from oracle import fill
from pytorch_segmentation_amd import models
from pytorch_segmentation_amd.utils import Trainer, compute_loss
rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
out = sys.argv[1]
torch.cuda.set_device(0)
dist.init_process_group('gloo', init_method='env://', world_size=world, rank=rank)
torch.manual_seed(100 + rank)
m = models.UNet(2)
if rank == 0:
    fill.fill_module_(m, 'dpmp/unet')
tr = Trainer(m, None, loss_fn=compute_loss, lr=1e-3, bucket_bytes=8 << 20, mixed_precision=True)
assert tr.reducer.enabled and tr.env.half
m.train()
states = []
for step in range(6):
    x = fill.images('dpmp/x%d' % step, (4 * world, 3, 128, 128))[4 * rank:4 * rank + 4].cuda()
    t = fill.labels('dpmp/t%d' % step, (4 * world, 128, 128), 2, block=8)[4 * rank:4 * rank + 4].cuda()
    if step == 2 and rank == 1:
        x = x * 3e4        # ONE rank's batch overflows fp16: its gradients go inf / nan, the all-reduce spreads that
    tr.train_batch(x, t)
    states.append(tr.loss_scale_state())
torch.cuda.synchronize()
torch.save({'params': tr.arena.params.cpu(), 'states': states}, '%s.rank%d.pt' % (out, rank))
dist.barrier()
dist.destroy_process_group()
'''


def test_two_rank_half_precision_skips_in_step(tmp_path):
    """The half-precision (-mp) policy under data parallelism (reference: apex amp + DistributedDataParallel inside the
    external Trainer, train.py:70,102-105,112-117): the overflow check runs on the REDUCED gradient arena, so when one rank's
    batch overflows fp16 every rank sees the inf / nan, every rank skips that step and halves its loss scale, and the
    replicas stay bit-identical.  Two processes on the test GPU, gradients over gloo."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'dpmp_worker.py'
    script.write_text(_MP_SCRIPT)
    out = str(tmp_path / 'dpmp')
    env = dict(os.environ, PSEG_REPO=repo)
    env.pop('PSEG_FORCE_REDUCER', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), str(script), out]
    r = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    r0, r1 = torch.load(out + '.rank0.pt'), torch.load(out + '.rank1.pt')
    assert r0['states'] == r1['states']                      # same scale, same applied / skipped counts after every step
    assert torch.equal(r0['params'], r1['params'])           # replicas bit-identical after six steps
    assert torch.isfinite(r0['params']).all()
    skipped = [s['steps_skipped'] for s in r0['states']]
    assert skipped[1] == 0 and skipped[2] == 1 and skipped[-1] == 1, skipped     # exactly the poisoned step was skipped ...
    assert r0['states'][2]['scale'] == 0.5 * r0['states'][1]['scale']             # ... and the scale halved, on both ranks
    assert r0['states'][-1]['steps_applied'] == 5


def test_two_rank_eval_uses_rank0_buffers(tmp_path):
    """2 ranks (gloo transport, both on the test GPU): after training on different data the replicas' running statistics
    differ; test() broadcasts rank 0's, so both ranks produce identical eval logits, hold rank 0's buffers afterwards, and
    the all-reduced mean IoU equals a single-process evaluation of rank 0's model over both shards."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'eval2.py'
    script.write_text(_EVAL_SCRIPT)
    out = str(tmp_path / 'res')
    env = dict(os.environ, PSEG_REPO=repo, PYTHONPATH=repo + os.pathsep + os.environ.get('PYTHONPATH', ''))
    env.pop('PSEG_FORCE_REDUCER', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), str(script), out]
    r = subprocess.run(cmd, cwd=repo, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = torch.load(out + '.rank0.pt'), torch.load(out + '.rank1.pt')
    assert any(not torch.equal(a['before'][k], b['before'][k]) for k in a['before'] if 'running_mean' in k)   # they DID differ
    for k in a['after']:
        assert torch.equal(a['after'][k], a['before'][k]), k           # rank 0 keeps its own
        assert torch.equal(b['after'][k], a['before'][k]), k           # rank 1 now holds rank 0's
    assert torch.equal(a['logits'], b['logits'])
    assert a['miou'] == b['miou']
    assert abs(a['miou'] - a['single']) < 1e-6, (a['miou'], a['single'])
