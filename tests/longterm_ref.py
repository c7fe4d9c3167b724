"""Plain numpy fp64 restatement of the long-term consistency loss (Ruder, Dosovitskiy & Brox
2016, eq. 9 and 10), built on tests/flow_ref.py: the yardstick of
tests/test_longterm_gpu.py, itself pinned by tests/test_longterm_host.py.

It is written as the paper writes it: the per-offset masks c^j, the long-term masks
c_long^j = max(c^j - sum_{k<j} c^k, 0), the per-offset warps, and a loss that is the explicit
sum over j.  It does not use the identity that ops.flow_compose rests on (the c_long^j are
mutually exclusive, so the sum is one masked loss on a composed reference); the host tests
check that identity against this file.

Lists are ordered nearest offset first: prevs[q] [n][c][h][w] is the result of frame
t - k_q, (fwds[q], bwds[q]) the flows between that frame and frame t."""
import numpy as np

import flow_ref as R


def long_masks(fwds, bwds):
    """(c_long [count][n][h][w] fp64 of 0 / 1, the per-offset flow_ref.consistency dicts)."""
    rs = [R.consistency(f, b) for f, b in zip(fwds, bwds)]
    cs = [r["c"].astype(np.float64) for r in rs]
    longs, nearer = [], np.zeros_like(cs[0])
    for c in cs:
        longs.append(np.maximum(c - nearer, 0.0))
        nearer = nearer + c
    return np.stack(longs), rs


def compose(prevs, fwds, bwds, fill):
    """dict: ref, init [n][c][h][w] fp64, cmask [n][h][w] fp64, which [n][h][w] uint8 (255: no
    offset), mag (sum_k |w_k a_k| of the selected warp, 0 elsewhere), rs (the per-offset
    consistency dicts, for their margins).  ref = sum_j c_long^j omega^j, cmask = sum_j
    c_long^j; init = ref where cmask, else the warp of prevs[0] along bwds[0] with fill."""
    longs, rs = long_masks(fwds, bwds)
    shape = np.asarray(prevs[0]).shape
    ref, mag = np.zeros(shape), np.zeros(shape)
    cmask = np.zeros(longs[0].shape)
    which = np.full(longs[0].shape, 255, np.uint8)
    for q, (p, b) in enumerate(zip(prevs, bwds)):
        om, _, m = R.warp(p, b, want_mag=True)
        on = longs[q] > 0
        ref += np.where(on[:, None], om, 0.0)  # (a select: an unselected warp may hold a NaN)
        mag += np.where(on[:, None], m, 0.0)
        cmask += longs[q]
        which[on] = q
    start, _ = R.warp(prevs[0], bwds[0], fill=fill)
    init = np.where(cmask[:, None] > 0, ref, start)
    return dict(ref=ref, cmask=cmask, init=init, which=which, mag=mag, rs=rs, longs=longs)


def long_loss(x, prevs, fwds, bwds, weight):
    """(L, sum|terms|): L = sum_j weight / (n c h w) sum_p c_long^j (x - omega^j)^2, the
    explicit sum over the offsets of flow_ref.masked_mse."""
    longs, _ = long_masks(fwds, bwds)
    total = mag = 0.0
    for q, (p, b) in enumerate(zip(prevs, bwds)):
        om, _ = R.warp(p, b)
        L, _, m = R.masked_mse(x, om, longs[q], weight)
        total += L
        mag += m
    return total, mag


# ------------------------------------------------------------------- the compose tests' inputs
SHAPES = [(1, 3, 5, 7), (2, 3, 33, 65), (1, 3, 64, 64)]  # (n, c, h, w)


def case(shape, count, seed=7):
    """(prevs, fwds, bwds, fill) fp32 for `count` offsets.  Offset q's flows are
    flow_ref.recipe(seed + q); an odd q takes the recipe reflected through the image centre
    (f'(i, j) = -f(h-1-i, w-1-j): an exact symmetry, which moves the occluded rectangle to
    the opposite quadrant, so the offsets disagree there).  On the last max(1, h // 6) rows
    offset q's backward flow leaves the image (dy = h) in the columns below w >> q: that band
    is handed from offset to offset, and its first w >> (count - 1) columns have no source."""
    n, c, h, w = shape
    rng = np.random.default_rng(100 + seed)
    prevs, fwds, bwds = [], [], []
    for q in range(count):
        fwd, bwd = R.recipe(h, w, seed=seed + q, n=n)
        if q % 2:
            fwd, bwd = (np.ascontiguousarray(-f[:, :, ::-1, ::-1]) for f in (fwd, bwd))
        bwd[:, 1, h - max(1, h // 6):, :w >> q] = h
        fwds.append(fwd)
        bwds.append(bwd)
        prevs.append(rng.uniform(-1, 1, shape).astype(np.float32))
    return prevs, fwds, bwds, rng.uniform(-1, 1, shape).astype(np.float32)


# ---------------------------------------------------------------------- the occlusion clip
CLIP_T, CLIP_H = 6, 64
OCC_W, OCC_SPEED, OCC_X0, OCC_ROWS = 6, 8, 4, (16, 48)


def occluder_cols(t):
    a = OCC_X0 + OCC_SPEED * t
    return a, a + OCC_W


def occlusion_clip(seed=91):
    """CLIP_T frames [1][3][64][64] fp32: a textured static background crossed by a textured
    occluder, OCC_W = 6 columns wide over rows 16..48, that moves OCC_SPEED = 8 columns per
    frame: narrower than its speed, so the columns it uncovers at frame t were visible at
    frame t-2."""
    rng = np.random.default_rng(seed)
    bg = rng.uniform(-1.5, 1.5, (1, 3, CLIP_H, CLIP_H)).astype(np.float32)
    occ = rng.uniform(-1.5, 1.5, (1, 3, OCC_ROWS[1] - OCC_ROWS[0], OCC_W)).astype(np.float32)
    frames = []
    for t in range(CLIP_T):
        f = bg.copy()
        a, b = occluder_cols(t)
        f[:, :, OCC_ROWS[0]:OCC_ROWS[1], a:b] = occ
        frames.append(f)
    return frames


def occlusion_flows(offsets=(1, 2)):
    """{k: (forward_k, backward_k)}, each [CLIP_T - k][2][64][64] fp32, the clip's exact
    flows: zero on the background; backward_k[t-k] is dx = -8 k on the occluder's pixels of
    frame t, forward_k[t-k] is dx = +8 k on its pixels of frame t-k."""
    out = {}
    for k in offsets:
        fwd = np.zeros((CLIP_T - k, 2, CLIP_H, CLIP_H), np.float32)
        bwd = np.zeros_like(fwd)
        for t in range(k, CLIP_T):
            a, b = occluder_cols(t)
            bwd[t - k, 0, OCC_ROWS[0]:OCC_ROWS[1], a:b] = -OCC_SPEED * k
            a, b = occluder_cols(t - k)
            fwd[t - k, 0, OCC_ROWS[0]:OCC_ROWS[1], a:b] = OCC_SPEED * k
        out[k] = (fwd, bwd)
    return out


def uncovered(flows, t):
    """m [1][64][64] bool at frame t >= 2: inconsistent with frame t-1 and consistent with
    frame t-2 -- the pixels only the long-term loss ties."""
    c1 = R.consistency(flows[1][0][t - 1:t], flows[1][1][t - 1:t])["c"]
    c2 = R.consistency(flows[2][0][t - 2:t - 1], flows[2][1][t - 2:t - 1])["c"]
    return ~c1 & c2


def uncovered_error(ys, flows):
    """mean over t >= 2 of sum m (y_t - W(y_{t-2}, bwd2_t))^2 / sum m, m = uncovered(t)."""
    errs = []
    for t in range(2, len(ys)):
        m = uncovered(flows, t)
        om, _ = R.warp(ys[t - 2], flows[2][1][t - 2:t - 1])
        d = np.where(m[:, None], np.asarray(ys[t], dtype=np.float64) - om, 0.0)
        errs.append(float((d * d).sum() / m.sum()))
    return float(np.mean(errs))
