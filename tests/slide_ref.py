"""Sliding-window inference restated for the tests (tests/test_slide_cpu.py, tests/test_slide_gpu.py): the window grid by
walking, not by formula, and the prediction in float64 -- accumulate and count per working pixel, divide, resize
bilinearly (align_corners=False) to the photo's size, sum over the scales, argmax with the first index winning ties."""
import torch
import torch.nn.functional as F


def work_size(H, W, s):
    """round half up of the scaled size, at least 1"""
    return max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))


def axis_origins(size, win, stride):
    """Walk the windows along one axis: step by the stride while the window ends inside the image, then one last window
    that ends exactly at the image's end; an image no longer than the window has the one window at 0."""
    if size <= win:
        return [0]
    out, o = [], 0
    while o + win < size:
        out.append(o)
        o += stride
    out.append(size - win)
    return out


def grid(Hs, Ws, h, w, sy, sx):
    """-> ([(y0, x0), ...] rows first, (ny, nx))"""
    ys, xs = axis_origins(Hs, h, sy), axis_origins(Ws, w, sx)
    return [(y0, x0) for y0 in ys for x0 in xs], (len(ys), len(xs))


def coverage(size, win, stride):
    """per pixel of one axis, the number of windows that contain it (counted one by one)"""
    return [sum(1 for o in axis_origins(size, win, stride) if o <= p < o + win) for p in range(size)]


def window_prob64(logits, pairs):
    """float64 [n,C,h,w]: the windows' softmax, plus the un-mirrored softmax of the mirrored twins (rows n..2n-1)"""
    p = torch.softmax(logits.double(), 1)
    if not pairs:
        return p
    n = logits.shape[0] // 2
    return p[:n] + p[n:].flip(3)


def working_prob64(p_wins, Hs, Ws, h, w, sy, sx):
    """float64 window probabilities [ny*nx,C,h,w] in (i, j) order -> ([C,Hs,Ws] mean over the covering windows, the
    integer count [Hs,Ws])"""
    origins, _ = grid(Hs, Ws, h, w, sy, sx)
    assert len(origins) == p_wins.shape[0]
    acc = torch.zeros(p_wins.shape[1], Hs, Ws, dtype=torch.float64)
    cnt = torch.zeros(Hs, Ws, dtype=torch.int64)
    for (y0, x0), p in zip(origins, p_wins):
        hh, ww = min(h, Hs - y0), min(w, Ws - x0)
        acc[:, y0:y0 + hh, x0:x0 + ww] += p[:, :hh, :ww]
        cnt[y0:y0 + hh, x0:x0 + ww] += 1
    assert (cnt >= 1).all()
    return acc / cnt.double(), cnt


def slide_oracle(work_probs, H, W):
    """[C,Hs,Ws] float64 per scale -> (argmax mask [H,W], top-2 margin of the summed resized probabilities)"""
    r = sum(F.interpolate(p[None], (H, W), mode='bilinear', align_corners=False)[0] for p in work_probs)
    if r.shape[0] == 1:
        return torch.zeros(H, W, dtype=torch.int64), torch.full((H, W), float('inf'), dtype=torch.float64)
    t = r.topk(2, dim=0).values
    return r.argmax(0), t[0] - t[1]
