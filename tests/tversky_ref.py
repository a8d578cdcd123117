"""The contract of pseg_tversky_fwd_bwd (include/pseg_amd.h) restated in numpy float64: loss, gradient with respect to the
logits, class_sums and the counts of out[].  tests/test_tversky_cpu.py holds it to finite differences and to torch autograd
in float64; tests/test_tversky_gpu.py holds the kernels to it."""
import numpy as np
import torch


def tversky_ref(logits, target, alpha=0.5, beta=0.5, smooth=1.0, power=1.0, per_image=False, all_classes=False,
                ignore_index=-100):
    """logits [B,C,H,W] (any float), target [B,H,W] int -> (loss, dlogits [B,C,H,W] float64, info).
    info: n_valid, n_bad, n_terms, n_groups (out[1:]), class_sums [G,C,3] = n_c, S_c, TP_c, terms [G,C] (NaN where the class
    is not counted), valid [B,H,W]."""
    x = np.asarray(logits, dtype=np.float64)
    B, C, H, W = x.shape
    t = np.asarray(target).reshape(B, H * W).astype(np.int64)
    z = x.reshape(B, C, H * W).transpose(0, 2, 1)                       # [B, HW, C]
    in_range = (t >= 0) & (t < C)
    valid = (t != ignore_index) & in_range
    ex = np.exp(z - z.max(2, keepdims=True))
    p = ex / ex.sum(2, keepdims=True)
    groups = [[b] for b in range(B)] if per_image else [list(range(B))]
    G = len(groups)
    sums = np.zeros((G, C, 3))
    terms = np.full((G, C), np.nan)
    per_group = []
    for g, imgs in enumerate(groups):
        v = valid[imgs].reshape(-1)
        pv, tv = p[imgs].reshape(-1, C)[v], t[imgs].reshape(-1)[v]
        onehot = np.zeros_like(pv)
        onehot[np.arange(len(tv)), tv] = 1.0
        n = onehot.sum(0)
        S = pv.sum(0)
        TP = (pv * onehot).sum(0)
        sums[g] = np.stack([n, S, TP], 1)
        counted = (np.ones(C, dtype=bool) if all_classes else n > 0) & (len(tv) > 0)
        FP, FN = S - TP, n - TP
        N = TP + smooth
        D = TP + alpha * FP + beta * FN + smooth
        TI = np.where(D == 0, 1.0, N / np.where(D == 0, 1.0, D))
        terms[g, counted] = (1 - TI[counted]) ** power
        per_group.append((imgs, v, pv, onehot, counted, N, D, FP, FN, TI))
    n_counted = np.array([int(pg[4].sum()) for pg in per_group])
    n_groups = int((n_counted > 0).sum())
    loss = 0.0
    dz = np.zeros_like(z)
    for g, (imgs, v, pv, onehot, counted, N, D, FP, FN, TI) in enumerate(per_group):
        if n_counted[g] == 0:
            continue
        loss += float(np.nansum(terms[g])) / n_counted[g] / n_groups
        K = np.zeros(C)
        pos = counted & (1 - TI > 0)
        K[pos] = -power * (1 - TI[pos]) ** (power - 1) / (n_counted[g] * n_groups)
        D2 = np.where(D == 0, 1.0, D) ** 2
        at_target = K * (beta * N + alpha * FP + beta * FN) / D2
        elsewhere = -K * alpha * N / D2
        gmat = onehot * at_target[None, :] + (1 - onehot) * elsewhere[None, :]
        dv = pv * (gmat - (gmat * pv).sum(1, keepdims=True))
        block = dz[imgs].reshape(-1, C)
        block[v] = dv
        dz[imgs] = block.reshape(len(imgs), H * W, C)
    info = {'n_valid': int(valid.sum()), 'n_bad': int(((t != ignore_index) & ~in_range).sum()),
            'n_terms': int(n_counted.sum()), 'n_groups': n_groups, 'class_sums': sums, 'terms': terms,
            'valid': valid.reshape(B, H, W)}
    return loss, dz.transpose(0, 2, 1).reshape(B, C, H, W).copy(), info


def make_case(B, C, H, W, std, seed, ignore_frac=0.1, n_bad=3, ignore_index=-100):
    """fp32 logits N(0, std), labels uniform over the classes, about ignore_frac of them ignore_index and n_bad (as far as
    there are pixels) out of range: C, -1, 1000, ..."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * std
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < ignore_frac] = ignore_index
    flat = target.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:min(n_bad, flat.numel() // 8)]
    flat[where] = torch.tensor([C, -1, 1000, C + 7, -5])[:len(where)] if len(where) else flat[where]
    return logits.float(), target
