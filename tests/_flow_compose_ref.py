"""CPU statements for the exact flow composition (include/microaligner_flowcompose.h):
(a) compose_flows_ref: the definition in numpy float32, one rounding per operation;
(b) register_exact: OptFlowRegistrator.register() with flow_composition = "exact" stated over the oracle's primitives
    (oracle/register_oracle.py, imported), i.e. the reference's level steps with only the bookkeeping of the flow changed.
TEST INFRASTRUCTURE, not product code."""
import numpy as np

from oracle import oracle as O
from oracle import register_oracle as RO

F32 = np.float32


def clamped_map(second):
    """(cx, cy) of steps 1-2: the sampling coordinate p - second(p), clamped to the image, NaN -> 0."""
    H, W = second.shape[:2]
    mx = np.arange(W, dtype=F32)[None, :] - second[..., 0]
    my = np.arange(H, dtype=F32)[:, None] - second[..., 1]
    with np.errstate(invalid="ignore"):
        cx = np.fmin(np.fmax(mx, F32(0)), F32(W - 1))
        cy = np.fmin(np.fmax(my, F32(0)), F32(H - 1))
    return cx.astype(F32), cy.astype(F32)


def compose_flows_ref(first, second):
    """out(p) = second(p) + first sampled at (p - second(p)): every operation on float32 arrays, so rounded on its own."""
    assert first.dtype == F32 and second.dtype == F32 and first.shape == second.shape and first.shape[2] == 2
    H, W = first.shape[:2]
    cx, cy = clamped_map(second)
    qx = np.rint(cx * F32(32)).astype(np.int64)    # half to even, as cvRound
    qy = np.rint(cy * F32(32)).astype(np.int64)
    ix, fx, iy, fy = qx >> 5, qx & 31, qy >> 5, qy & 31
    ix1, iy1 = np.minimum(ix + 1, W - 1), np.minimum(iy + 1, H - 1)
    s = F32(1.0 / 32.0)
    x1 = fx.astype(F32) * s
    x0 = F32(1) - x1
    y1 = fy.astype(F32) * s
    y0 = F32(1) - y1
    w = [(y0 * x0)[..., None], (y0 * x1)[..., None], (y1 * x0)[..., None], (y1 * x1)[..., None]]
    v = [first[iy, ix], first[iy, ix1], first[iy1, ix], first[iy1, ix1]]
    with np.errstate(invalid="ignore", over="ignore"):
        acc = v[0] * w[0]
        for k in (1, 2, 3):
            acc = acc + v[k] * w[k]
        out = second + acc
    assert out.dtype == F32
    return out


def register_exact(ref, mov, num_pyr_lvl=4, num_iterations=3, tile_size=1000, overlap=100, use_full_res_img=False,
                   use_dog=False, fused=False, nthreads=1, dog_flags=0, compose=compose_flows_ref):
    """(flow, reports) with reports = [(factor, mi_after, mi_before, accepted), ...]: the level steps of
    register_oracle.register (warp, dog, Farneback, warp, gate) and, per level, with t this level's flow and m the flow
    so far:  total T = t (level 0) or compose(m, t) if accepted, zeros (level 0) or m if rejected;
    then m = pyrUp(T * 2, next level's size), or at the last level return T (full-resolution level) or
    pyrUp(T * 2, full size)."""
    win = overlap - (1 - overlap % 2)
    O.set_threads(nthreads)
    ref_pyr, factors = RO.image_pyramid(ref, num_pyr_lvl, use_full_res_img)
    mov_pyr, _ = RO.image_pyramid(mov, num_pyr_lvl, use_full_res_img)
    n = len(factors)
    reports, m_flow = [], None
    for lvl, factor in enumerate(factors):
        last = lvl == n - 1
        mov_lvl = mov_pyr[lvl].copy()
        if lvl > 0:
            mov_lvl = RO.warp(mov_lvl, m_flow, tile_size, overlap)
        fb_ref, fb_mov = O.dog(ref_pyr[lvl], use_dog, flags=dog_flags), O.dog(mov_lvl, use_dog, flags=dog_flags)
        this_flow = RO.tile_flow(fb_ref, fb_mov, tile_size, overlap, win, num_iterations, fused=fused, nthreads=nthreads)
        warped = RO.warp(mov_lvl, this_flow, tile_size, overlap)
        ref_d = O.dog(ref_pyr[lvl], True, flags=dog_flags)
        after = RO.mi_tiled(ref_d, O.dog(warped, True, flags=dog_flags), tile_size)
        before = RO.mi_tiled(ref_d, O.dog(mov_pyr[lvl], True, flags=dog_flags), tile_size)
        ok = bool(after > before)
        reports.append((factor, float(after), float(before), ok))
        if ok:
            total = this_flow if lvl == 0 else compose(m_flow, this_flow)
        else:
            total = np.zeros(this_flow.shape, F32) if lvl == 0 else m_flow
        if not last:
            m_flow = O.pyr_up(total * 2, dstsize=mov_pyr[lvl + 1].shape[::-1])
        elif use_full_res_img:
            m_flow = total
        else:
            m_flow = O.pyr_up(total * 2, dstsize=ref.shape[::-1])
    return m_flow, reports


def endpoint_error(flow, truth, border=64):
    """median, 99th percentile and max of |flow - truth| in px, `border` px left out on every side."""
    d = (flow.astype(np.float64) - truth)[border:-border, border:-border]
    e = np.hypot(d[..., 0], d[..., 1])
    return float(np.median(e)), float(np.percentile(e, 99)), float(e.max())
