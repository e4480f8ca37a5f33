"""float64 restatement of the error-map importance sampling (``ErrorMap`` / ``ImpSampler`` of
nr3d_lib.models.importance, the kernels ``nsim_errmap_*`` of csrc/sampling.hip) in plain torch -- the checker of
tests/test_importance.py.  It takes the f32 inputs the kernels take and computes everything else in float64.

The one thing kept in f32 is the CELL of a pixel, ``cx = clamp(int(x w), 0, w - 1)`` with the product rounded to f32: that is the
definition of the cell (the torch classes and the kernels both evaluate it so), not a matter of precision -- a pixel on a cell
border belongs to one cell, and the float64 product would put a few of them into the neighbour."""
import torch

EPS24 = 2.0 ** -24
XY_LO, XY_HI = float(torch.tensor(1e-6, dtype=torch.float32)), float(torch.tensor(1 - 1e-6, dtype=torch.float32))


def cells(fidx, xy, h: int, w: int):
    """-> (flat cell index [N] int64 into [n_images, h, w], cx, cy)"""
    xy = xy.detach().cpu().float().reshape(-1, 2)
    fidx = fidx.detach().cpu().long().reshape(-1)
    if fidx.numel() == 1 and xy.shape[0] > 1:
        fidx = fidx.expand(xy.shape[0])
    cx = (xy[:, 0] * w).long().clamp(0, w - 1)
    cy = (xy[:, 1] * h).long().clamp(0, h - 1)
    return (fidx * h + cy) * w + cx, cx, cy


def rgb_error(pred, gt, fn: str):
    """mean_c fn(pred - gt) [N] in float64 (app/loss/photometric.py:111-112)"""
    d = pred.detach().cpu().double() - gt.detach().cpu().double()
    return (d.abs() if fn == "l1" else d * d).mean(-1)


def update(em, n_steps, fidx, xy, val):
    """ErrorMap.step_error_map on a float64 map [V, h, w]: -> (new map float64, new n_steps, per-cell counts [V, h, w] int64)"""
    V, h, w = em.shape
    flat, _, _ = cells(fidx, xy, h, w)
    val = val.detach().cpu().double().reshape(-1)
    s = torch.zeros([V * h * w], dtype=torch.float64).index_add_(0, flat, val)
    c = torch.zeros([V * h * w], dtype=torch.float64).index_add_(0, flat, torch.ones_like(val))
    out = em.detach().cpu().double().reshape(-1).clone()
    hit = c > 0
    out[hit] = 0.5 * out[hit] + 0.5 * (s[hit] / c[hit])
    ns = n_steps.detach().cpu().long().clone()
    ns[torch.unique(torch.div(flat, h * w, rounding_mode="floor"))] += 1
    return out.view(V, h, w), ns, c.long().view(V, h, w)


def pdf(em, min_pdf: float, max_pdf=None):
    """ErrorMap.get_pdf in float64: [V, h, w], every image summing to 1"""
    V, h, w = em.shape
    p = em.detach().cpu().double().clamp_min(0) + 1e-12
    p = p / p.sum(dim=(-2, -1), keepdim=True)
    p = p.clamp_min(float(torch.tensor(min_pdf, dtype=torch.float32)) / (h * w))
    if max_pdf is not None:
        p = p.clamp_max(max(float(max_pdf), 1.0))
    return p / p.sum(dim=(-2, -1), keepdim=True)


def cdf_cell(em, min_pdf: float, max_pdf=None):
    """[V, h w] float64 inclusive scan of ``pdf``"""
    return pdf(em, min_pdf, max_pdf).reshape(em.shape[0], -1).cumsum(-1)


def pdf_image(em):
    m = em.detach().cpu().double().sum(dim=(-2, -1))
    return m / m.sum().clamp_min(1e-12)


def cdf_image(em):
    return pdf_image(em).cumsum(0)


def uniform_rows(u, V: int):
    """the uniform formula of a draw: fidx = min(int(u0 V), V - 1) with the product in f32, xy = clamp((u2, u3))"""
    u = u.detach().cpu().float()
    fidx = (u[:, 0] * V).long().clamp(0, V - 1)
    return fidx, u[:, 2:4].clamp(XY_LO, XY_HI)
