"""The scene-flow field of the EmerNeRF dynamic model (``use_flow_field``) against the float64 restatement
tests/dynamic_flow_ref.py: ``nsim_permuto_dx_pts`` -- the gradient of the point-mode lattice gather to its input points, which a
flow-warped query needs because its lattice points are network outputs --, the flow decoder (``nsim_flow_fwd`` / ``_bwd``), the warp,
the whole with-flow model (``nsim_dyn_fwd_agg`` / ``_bwd_agg``), its configuration, and ``losses.flow_loss`` / ``flow_block_terms``
(``nsim_flow_loss_fwd`` / ``_bwd``), the cycle and sparsity terms of app/loss/flow.py, also against the reference's own class."""
import pytest
import torch

import dynamic_flow_ref as fref
from conftest import sync
from oracle import permuto as operm
from util import leaf, rel_l2

# ------------------------------------------------------------------------------------------------ 1. nsim_permuto_dx_pts
DX_CFG = dict(n_feats=2, coarsest_res=2.0, finest_res=24.0, seed=3)
MIN_GAP, MAX_EXCLUDED = 1e-4, 0.02
# (L, S) -> (seed, excluded points): the first seed whose points leave at most 2 % of them within 1e-4 of a simplex face on some
# level (where d h / d x jumps), and the points left out at that seed -- chosen by tests/dynamic_flow_ref.py alone, on the CPU
DX_CASES = {
    (1, 1): (0, []), (1, 31): (0, []), (1, 32): (0, []), (1, 33): (0, []), (1, 257): (0, []),
    (6, 1): (0, []), (6, 31): (1, []), (6, 32): (1, []), (6, 33): (0, []), (6, 257): (0, [66]),
    (16, 1): (0, []), (16, 31): (2, []), (16, 32): (3, []), (16, 33): (0, []), (16, 257): (5, [52, 194, 210, 213, 253]),
}
# f32 products of exact constants (d bary / d x = scale / 5), fp16-exact table values and the f32 dh, summed in f32 over at most
# 16 levels x 5 vertices x 2 features: the bound of the lattice family's f32 gradients (tests/test_permuto_distant.py)
DX_TOL = 2e-5


def _dx_call(pc, table16, x, valid, dh_pl, pitch, backend):
    from neuralsim_amd import _lib
    S = x.shape[0]
    dx = torch.empty([S, 4], dtype=torch.float32, device=backend)          # (NaN-poisoned: every row must be written)
    _lib.call("nsim_permuto_dx_pts", pc.meta, _lib.ptr(table16.to(backend)), _lib.ptr(x.to(backend).contiguous()),
              _lib.ptr(None if valid is None else valid.to(torch.uint8).to(backend)), S, _lib.ptr(dh_pl.to(backend)), pitch,
              _lib.ptr(dx))
    sync(backend)
    return dx.cpu()


def _planes(dh, L, pitch, rows=None):
    """dh [S, 2 L] -> level-major planes [16][pitch][2]; everything the kernel must not read is NaN"""
    S = dh.shape[0]
    pl = torch.full([16, pitch, 2], float("nan"))
    rows = L if rows is None else rows
    pl[:rows, :S] = dh.view(S, L, 2).permute(1, 0, 2)[:rows]
    return pl


@pytest.mark.parametrize("log2_T", [4, 10])
@pytest.mark.parametrize("S", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("L", [1, 6, 16])
def test_permuto_dx_pts(backend, L, S, log2_T):
    """dx = d (dh . h(x)) / d x over all four inputs against float64 autograd of the restated lattice: every point, a valid mask
    with zeros (those rows exactly 0, their dh rows NaN), a hard level mask (the masked levels' tables and dh planes NaN), a plane
    pitch above S.  2^4 entries: every vertex collides; 2^10: the size of the model tests."""
    from neuralsim_amd.grid_encodings.permuto import PermutoConfig
    pc = PermutoConfig(in_dim=4, n_levels=L, log2_hashmap_size=log2_T, **DX_CFG)
    spec = operm.make_permuto_spec(in_dim=4, n_levels=L, log2_hashmap_size=log2_T, **DX_CFG)
    seed, x, excl = fref.pick_dx_seed(S, spec, MIN_GAP, MAX_EXCLUDED)
    share = float(excl.float().mean())
    print(f"L {L} S {S}: seed {seed}, excluded {excl.nonzero()[:, 0].tolist()} ({share:.4f})")
    assert share <= MAX_EXCLUDED and (seed, excl.nonzero()[:, 0].tolist()) == DX_CASES[(L, S)]
    keep = ~excl
    g = torch.Generator().manual_seed(7 * L + S + log2_T)
    table = ((torch.rand(spec.n_params, generator=g) * 2 - 1) * 0.5).half()
    dh = torch.randn(S, 2 * L, generator=g)
    # -- every point, pitch S
    ref = fref.dx_pts(x, table, spec, dh)
    assert float(ref.abs().max()) > 0
    got = _dx_call(pc, table, x, None, _planes(dh, L, S), 0, backend)
    e = rel_l2(got[keep], ref[keep])
    print(f"  all points: rel-L2 {e:.2e}")
    assert e < DX_TOL
    # -- a valid mask with zeros, pitch S + 5 (the rows of another point set behind this one's)
    valid = torch.rand(S, generator=g) > 1.0 / 3.0
    if S == 1:
        valid[:] = False
    else:
        valid[0], valid[-1] = False, True
    dh_m = dh.clone()
    dh_m[~valid] = float("nan")
    got = _dx_call(pc, table, x, valid, _planes(dh_m, L, S + 5), S + 5, backend)
    assert torch.equal(got[~valid], torch.zeros(int((~valid).sum()), 4))
    sel = keep & valid
    if bool(sel.any()):
        e = rel_l2(got[sel], ref[sel])
        print(f"  valid mask: rel-L2 {e:.2e}")
        assert e < DX_TOL
    # -- a hard level mask
    if L > 1:
        na = L // 2
        T2 = 2 * spec.hashmap_size
        table_m = table.clone()
        table_m[na * T2:] = float("nan")
        ref_m = fref.dx_pts(x, table_m, spec, dh, n_active=na)
        assert bool(torch.isfinite(ref_m).all())
        pc.meta.n_active_levels = na
        try:
            got = _dx_call(pc, table_m, x, None, _planes(dh, L, S, rows=na), 0, backend)
        finally:
            pc.meta.n_active_levels = 0
        e = rel_l2(got[keep], ref_m[keep])
        print(f"  {na} of {L} levels: rel-L2 {e:.2e}")
        assert e < DX_TOL


def test_permuto_dx_pts_arguments(backend):
    """S == 0 launches nothing; a pitch below S, a table of more than 16 levels and a missing plane pointer are refused"""
    from neuralsim_amd import _lib
    from neuralsim_amd.grid_encodings.permuto import PermutoConfig
    pc = PermutoConfig(in_dim=4, n_levels=2, log2_hashmap_size=4, **DX_CFG)
    t16 = torch.zeros(2 * 16 * 2, dtype=torch.float16, device=backend)
    x = torch.zeros(3, 4, device=backend)
    pl = torch.zeros(16, 3, 2, device=backend)
    dx = torch.zeros(3, 4, device=backend)
    _lib.call("nsim_permuto_dx_pts", pc.meta, _lib.ptr(t16), _lib.ptr(x), None, 0, _lib.ptr(pl), 0, _lib.ptr(dx))
    with pytest.raises(RuntimeError):
        _lib.call("nsim_permuto_dx_pts", pc.meta, _lib.ptr(t16), _lib.ptr(x), None, 3, _lib.ptr(pl), 2, _lib.ptr(dx))
    with pytest.raises(RuntimeError):
        _lib.call("nsim_permuto_dx_pts", pc.meta, _lib.ptr(t16), _lib.ptr(x), None, 3, None, 0, _lib.ptr(dx))
    pc17 = PermutoConfig(in_dim=4, n_levels=17, log2_hashmap_size=4, **DX_CFG)
    with pytest.raises(RuntimeError):
        _lib.call("nsim_permuto_dx_pts", pc17.meta, _lib.ptr(t16), _lib.ptr(x), None, 3, _lib.ptr(pl), 0, _lib.ptr(dx))


def test_forward_planes_autograd(backend):
    """``PermutoEncoding.forward_planes``: the planes, and through autograd the gradients to the table and to points that are
    themselves a function of a parameter (x = x0 + shift: what a flow-warped query hands the lattice); the backward runs under the
    level mask of the forward even when the mask has changed in between"""
    from neuralsim_amd.grid_encodings.permuto import PermutoEncoding
    L, S = 6, 257
    cfg = dict(n_levels=L, log2_hashmap_size=10, **DX_CFG)
    spec = operm.make_permuto_spec(in_dim=4, **cfg)
    seed, x0, excl = fref.pick_dx_seed(S, spec, MIN_GAP, MAX_EXCLUDED)
    keep = ~excl
    enc = PermutoEncoding(4, permuto_auto_compute_cfg=dict(cfg), bound=0.5, seed=5).to(backend)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(S, 2 * L, generator=g)
    w[excl] = 0.0                                # (points on a face: no statement about their share of any gradient)
    for na in (0, 3):
        table64 = leaf(enc.flattened_params.cpu(), dtype=torch.float64)
        shift64 = torch.zeros(4, dtype=torch.float64, requires_grad=True)
        ref = fref.active_features(x0.double() + shift64, table64, spec, na or None)
        (ref * w.double()).sum().backward()
        enc.zero_grad()
        shift = torch.zeros(4, device=backend, requires_grad=True)
        enc.cfg.meta.n_active_levels = na
        try:
            pl = enc.forward_planes(x0.to(backend) + shift)
        finally:
            enc.cfg.meta.n_active_levels = 0      # the mask changes before the backward
        assert pl.shape == (16, S, 2) and not bool(pl[L:].any())
        got = pl[:L].permute(1, 0, 2).reshape(S, 2 * L)
        err = float((got.detach().cpu().double() - ref.detach()).abs().max())
        assert err < 2e-5 * (1 + float(ref.detach().abs().max()))
        (got * w.to(backend)).sum().backward()
        sync(backend)
        e_t, e_s = rel_l2(enc.flattened_params.grad.cpu(), table64.grad), rel_l2(shift.grad.cpu(), shift64.grad)
        print(f"n_active {na}: planes {err:.2e}, d table {e_t:.2e}, d shift {e_s:.2e}")
        assert e_t < DX_TOL and e_s < DX_TOL
        if na:
            assert not bool(enc.flattened_params.grad[na * 2 * spec.hashmap_size:].any())
    with pytest.raises(ValueError):
        enc.forward_planes(torch.zeros(3, 3, device=backend))


# ------------------------------------------------------------------------------------------------ 2. flow decoder, warp
# the bounds of the decoder family (tests/test_nerf.py / test_dynamic_nerf.py::test_decoder_parity): values 2e-5 (f32) | 5e-3 (fp16)
# of 1 + max |value|, gradients 3e-4 | 6.24e-2 relative L2
VAL_TOL, GRAD_TOL = dict(f32=2e-5, fp16=5e-3), dict(f32=3e-4, fp16=6.24e-2)


def _flow_pack(L, prec, fw, fb, backend):
    from neuralsim_amd import _lib
    n = int(_lib.get_lib().nsim_flow_wpack_bytes(prec))
    assert n > 0
    wpack = torch.zeros([n], dtype=torch.uint8, device=backend)
    _lib.call("nsim_flow_pack_weights", L, prec, _lib.ptr(fw.to(backend)), _lib.ptr(fb.to(backend)), _lib.ptr(wpack))
    return wpack


@pytest.mark.parametrize("S", [1, 31, 32, 33, 257])
@pytest.mark.parametrize("L", [1, 6, 16])
@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_flow_decoder(backend, precision, L, S):
    """flow6 and the gradients to flow_w, flow_b and the feature planes against float64; a plane pitch above S (the rows of other
    point sets in one buffer), planes past the lattice's levels NaN (never read), dh rows of those levels left alone"""
    from neuralsim_amd import _lib
    prec = dict(fp16=0, f32=1)[precision]
    pitch = S if L == 6 else S + 3
    g = torch.Generator().manual_seed(100 * L + S)
    h = (torch.rand(S, 2 * L, generator=g) * 2 - 1) * 0.5
    fw, fb = fref.make_flow_decoder(L)
    gout = torch.randn(S, 6, generator=g)
    h64, w64, b64 = leaf(h, dtype=torch.float64), leaf(fw, dtype=torch.float64), leaf(fb, dtype=torch.float64)
    ref = fref.flow_decoder(h64, w64, b64)
    (ref * gout.double()).sum().backward()
    wpack = _flow_pack(L, prec, fw, fb, backend)
    h_pl = _planes(h, L, pitch).to(backend)
    flow6 = torch.empty([S, 6], dtype=torch.float32, device=backend)
    _lib.call("nsim_flow_fwd", L, prec, _lib.ptr(wpack), _lib.ptr(h_pl), pitch, S, _lib.ptr(flow6))
    sync(backend)
    ev = float((flow6.cpu().double() - ref.detach()).abs().max()) / (1 + float(ref.detach().abs().max()))
    dw = torch.zeros_like(fw).to(backend)
    db = torch.zeros_like(fb).to(backend)
    dh_pl = torch.empty([16, pitch, 2], dtype=torch.float32, device=backend)
    _lib.call("nsim_flow_bwd", L, prec, _lib.ptr(wpack), _lib.ptr(h_pl), pitch, S, _lib.ptr(gout.to(backend)), _lib.ptr(dh_pl),
              _lib.ptr(dw), _lib.ptr(db))
    sync(backend)
    dh = dh_pl.cpu()[:L, :S].permute(1, 0, 2).reshape(S, 2 * L)
    eg = dict(flow_w=rel_l2(dw.cpu(), w64.grad), flow_b=rel_l2(db.cpu(), b64.grad), dh=rel_l2(dh, h64.grad))
    print(f"[flow decoder {precision} L={L} S={S}] value {ev:.2e}", {k: f"{v:.2e}" for k, v in eg.items()})
    assert ev < VAL_TOL[precision]
    for k, e in eg.items():
        assert e < GRAD_TOL[precision], (k, e)
    assert bool(torch.isnan(dh_pl.cpu()[L:]).all()) and bool(torch.isnan(dh_pl.cpu()[:, S:]).all())
    # without a consumer of the plane gradient the weight gradients are the same
    dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
    _lib.call("nsim_flow_bwd", L, prec, _lib.ptr(wpack), _lib.ptr(h_pl), pitch, S, _lib.ptr(gout.to(backend)), None, _lib.ptr(dw2),
              _lib.ptr(db2))
    assert rel_l2(dw2.cpu(), w64.grad) < GRAD_TOL[precision] and rel_l2(db2.cpu(), b64.grad) < GRAD_TOL[precision]


def test_flow_decoder_arguments(backend):
    from neuralsim_amd import _lib
    assert int(_lib.get_lib().nsim_flow_wpack_bytes(2)) == -1
    fw, fb = fref.make_flow_decoder(2)
    wpack = _flow_pack(2, 1, fw, fb, backend)
    pl, out = torch.zeros(16, 3, 2, device=backend), torch.zeros(3, 6, device=backend)
    _lib.call("nsim_flow_fwd", 2, 1, _lib.ptr(wpack), _lib.ptr(pl), 0, 0, _lib.ptr(out))          # S == 0: nothing
    for bad in ((17, 1, 0), (0, 1, 0), (2, 3, 0), (2, 1, 2)):                                      # levels, precision, pitch < S
        with pytest.raises(RuntimeError):
            _lib.call("nsim_flow_fwd", bad[0], bad[1], _lib.ptr(wpack), _lib.ptr(pl), bad[2], 3, _lib.ptr(out))
    with pytest.raises(RuntimeError):
        _lib.call("nsim_flow_bwd", 2, 1, _lib.ptr(wpack), _lib.ptr(pl), 0, 3, _lib.ptr(out), None, None, None)


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("S", [1, 257])
def test_dyn_warp(backend, S, T):
    """the warped lattice points, bit for bit (one f32 add each), with time codes on both ends of the range so both clamps are hit;
    the backward adds the position parts into dflow6"""
    from neuralsim_amd import _lib
    g = torch.Generator().manual_seed(S + T)
    codes = torch.linspace(-1.0, 1.0, T) if T > 1 else torch.tensor([-1.0])
    x4 = torch.cat([torch.rand(S, 3, generator=g) * 4 - 2, codes[torch.arange(S) % T][:, None]], dim=1)
    if S > 1:
        x4[0, 3], x4[1, 3] = codes[0], codes[-1]
    flow6 = torch.randn(S, 6, generator=g) * 0.3
    delta, _, _ = fref.time_neighbours(x4[:, 3], T)
    want = fref.warp(x4, flow6, torch.tensor(delta, dtype=torch.float32), -1.0, 1.0)
    got = torch.empty([2 * S, 4], dtype=torch.float32, device=backend)
    _lib.call("nsim_dyn_warp_fwd", _lib.ptr(x4.to(backend)), _lib.ptr(flow6.to(backend)), S, float(delta), -1.0, 1.0, _lib.ptr(got))
    sync(backend)
    assert torch.equal(got.cpu(), want)
    assert float(got[:S, 3].max()) <= 1.0 and float(got[S:, 3].min()) >= -1.0
    if T == 1:
        assert torch.equal(got.cpu()[:S, 3], x4[:, 3]) and torch.equal(got.cpu()[S:, 3], x4[:, 3])
    dx = torch.randn(2 * S, 4, generator=g)
    d0 = torch.randn(S, 6, generator=g)
    d = d0.clone().to(backend)
    _lib.call("nsim_dyn_warp_bwd", _lib.ptr(dx.to(backend)), S, _lib.ptr(d))
    sync(backend)
    assert torch.equal(d.cpu(), d0 + torch.cat([dx[:S, :3], dx[S:, :3]], dim=1))


# ------------------------------------------------------------------------------------------------ 6. flow_loss
# The kernels sum in f64 and round once to f32; the restatement is f64 on the same f32 inputs.  One f32 rounding: 2^-24 relative for
# the values, and for the gradients a further one of the f32 upstream gradient the autograd engine hands over -- 2^-23.
FLOW_ULP = 2.0 ** -23
FLOW_KEYS = ("flow_fwd", "flow_fwd_pred_bwd", "flow_bwd", "flow_bwd_pred_fwd")


def _flow_inputs(S, seed=0):
    """four [S,3] f32 tensors; from S >= 2 on rows that are exactly zero: one tensor at a time, and all four at once"""
    g = torch.Generator().manual_seed(seed + S)
    ts = [torch.randn(S, 3, generator=g) * (0.05 * (k + 1)) for k in range(4)]
    if S >= 63:
        for k in range(4):
            ts[k][3 + 5 * k] = 0.0
        for k in range(4):
            ts[k][40] = 0.0
    return ts


def _flow_ref(ts, w_cycle, w_sparsity, a, b):
    ls = [leaf(t, dtype=torch.float64) for t in ts]
    cyc, spa = fref.flow_loss(*ls, w_cycle=w_cycle, w_sparsity=w_sparsity)
    (a * cyc + b * spa).backward()
    return cyc.detach(), spa.detach(), [t.grad if t.grad is not None else torch.zeros_like(t) for t in ls]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 4097])
def test_flow_loss(backend, S):
    from neuralsim_amd import losses
    ts = _flow_inputs(S)
    wc, wsp, a, b = 0.75, 0.01, 2.0, 0.5                   # (the upstream gradients a, b are exact in f32)
    cyc64, spa64, g64 = _flow_ref(ts, wc, wsp, a, b)
    assert bool(torch.isfinite(torch.stack([cyc64, spa64])).all()) and all(bool(torch.isfinite(g).all()) for g in g64)
    ls = [leaf(t, backend) for t in ts]
    cyc, spa = losses.flow_loss(*ls, w_cycle=wc, w_sparsity=wsp)
    assert cyc.dtype == torch.float32 and cyc.shape == () and spa.shape == ()
    (a * cyc + b * spa).backward()
    sync(backend)
    for name, v, v64 in (("cycle", cyc, cyc64), ("sparsity", spa, spa64)):
        e = abs(float(v.detach().cpu().double()) - float(v64))
        print(f"S {S} {name}: {float(v64):.6e} err {e:.2e}")
        assert e <= FLOW_ULP * abs(float(v64))
    for k, (t, g) in enumerate(zip(ls, g64)):
        got = t.grad.cpu().double()
        assert bool(torch.isfinite(got).all()), FLOW_KEYS[k]
        e = float((got - g).abs().max())
        print(f"S {S} d {FLOW_KEYS[k]}: max err {e:.2e} of {float(g.abs().max()):.2e}")
        assert e <= FLOW_ULP * float(g.abs().max()), FLOW_KEYS[k]
        zero_rows = (ts[k] == 0).all(dim=1)
        if k in (0, 2):         # the stop-gradient operands: the sparsity term alone -- a zero row gets exactly zero
            assert torch.equal(got[zero_rows], torch.zeros(int(zero_rows.sum()), 3, dtype=torch.float64))
    if S >= 63:
        assert all(int((t == 0).all(dim=1).sum()) == 2 for t in ts)


def test_flow_loss_stop_gradient(backend):
    """flow_fwd / flow_bwd get nothing from the cycle term and their norm's gradient from the sparsity term; a term nobody
    differentiates costs nothing: its upstream gradient is absent, not zero-filled"""
    from neuralsim_amd import losses
    ts = _flow_inputs(65, seed=3)
    ls = [leaf(t, backend) for t in ts]
    cyc, _ = losses.flow_loss(*ls, w_cycle=1.0, w_sparsity=1.0)
    cyc.backward()
    sync(backend)
    assert not bool(ls[0].grad.any()) and not bool(ls[2].grad.any())
    assert bool(ls[1].grad.any()) and bool(ls[3].grad.any())
    _, _, g64 = _flow_ref(ts, 1.0, 1.0, 1.0, 0.0)
    for k in (1, 3):
        assert float((ls[k].grad.cpu().double() - g64[k]).abs().max()) <= FLOW_ULP * float(g64[k].abs().max())
    ls = [leaf(t, backend) for t in ts]
    _, spa = losses.flow_loss(*ls, w_cycle=1.0, w_sparsity=1.0)
    spa.backward()
    sync(backend)
    _, _, g64 = _flow_ref(ts, 1.0, 1.0, 0.0, 1.0)
    for k in range(4):
        assert bool(ls[k].grad.any())
        assert float((ls[k].grad.cpu().double() - g64[k]).abs().max()) <= FLOW_ULP * float(g64[k].abs().max())
    # only the predictions require a gradient: the other two outputs are not written
    ls = [t.to(backend) for t in ts]
    ls[1].requires_grad_(True)
    cyc, spa = losses.flow_loss(*ls)
    (cyc + spa).backward()
    assert ls[0].grad is None and ls[1].grad is not None


def test_flow_loss_empty_and_shapes(backend, monkeypatch):
    """S == 0: zeros without a launch; [..., 3] inputs keep their shape in the gradient; mismatched shapes are refused"""
    from neuralsim_amd import _lib, losses
    e = [torch.zeros(0, 3, device=backend, requires_grad=True) for _ in range(4)]
    monkeypatch.setattr(_lib, "CALL_COUNT", 0)
    cyc, spa = losses.flow_loss(*e, w_cycle=2.0, w_sparsity=3.0)
    n = _lib.CALL_COUNT
    monkeypatch.setattr(_lib, "CALL_COUNT", None)
    assert n == 0 and float(cyc) == 0.0 and float(spa) == 0.0 and cyc.dtype == torch.float32
    ts = [t.view(5, 13, 3) for t in _flow_inputs(65, seed=5)]
    ls = [leaf(t, backend) for t in ts]
    monkeypatch.setattr(_lib, "CALL_COUNT", 0)
    cyc, spa = losses.flow_loss(*ls)
    (cyc + spa).backward()
    n = _lib.CALL_COUNT
    monkeypatch.setattr(_lib, "CALL_COUNT", None)
    assert n == 2                                          # one launch per direction for both terms
    assert all(t.grad.shape == (5, 13, 3) for t in ls)
    c64, s64, _ = _flow_ref([t.reshape(-1, 3) for t in ts], 1.0, 1.0, 1.0, 1.0)
    assert abs(float(cyc.detach()) - float(c64)) <= FLOW_ULP * float(c64) and abs(float(spa.detach()) - float(s64)) <= FLOW_ULP * float(s64)
    with pytest.raises(ValueError):
        losses.flow_loss(ls[0], ls[1], ls[2], ls[3][:4])
    with pytest.raises(ValueError):
        losses.flow_loss(*[t[..., :2] for t in ls])


# ------------------------------------------------------------------------------------------------ 7. the ``flow`` block
import json                # noqa: E402
import sys                 # noqa: E402
from pathlib import Path   # noqa: E402

import ref_glue            # noqa: E402

FLOW_FIXTURE = Path(__file__).resolve().parent / "golden" / "flow_loss_fixture.json"
needs_reference = ref_glue.needs_reference(ref_glue.readable(ref_glue.REF_ROOT / "app" / "loss" / "flow.py"),
                                           reason="executes the reference's own FlowLoss (emulator backend only); what it pins is "
                                                  "replayed from tests/golden/flow_loss_fixture.json on both backends")
# a term is a mean of at most 333 x 3 f32 products that torch sums in f32: the reference's own departure from its float64 run is
# the scale of the bound (4 x), with a floor of 2 f32 ulps of the value for the terms torch happens to round exactly
BLOCK_MARGIN, BLOCK_FLOOR = 4.0, 2.0 ** -22


def _block_check(case, got: dict, want: dict):
    """want: key -> [float64 value, float32 value] of the reference"""
    assert list(got) == list(want), (case, list(got), list(want))
    for k, (v64, v32) in want.items():
        v = got[k]
        assert v.dtype == torch.float32 and v.shape == ()
        e, tol = abs(float(v.detach().cpu().double()) - v64), max(BLOCK_MARGIN * abs(v32 - v64), BLOCK_FLOOR * abs(v64))
        print(f"{case} {k}: {v64:.6e} err {e:.2e} (reference f32 {abs(v32 - v64):.2e}, bound {tol:.2e})")
        assert e <= tol, (case, k, e, tol)


def _block_run(case, backend):
    from neuralsim_amd import losses
    block, it = fref.FLOW_BLOCK_CASES[case]
    raw, uni = fref.flow_block_inputs(torch.float32, backend)
    leaves = [t.requires_grad_(True) for o in list(raw.values()) + [dict(volume_buffer=u) for u in uni.values()]
              for k, t in o["volume_buffer"].items() if k in fref.FLOW_KEYS]
    out = losses.flow_block_terms(block, raw, uni, it)
    sum(out.values()).backward()
    sync(backend)
    assert all(t.grad is None or bool(torch.isfinite(t.grad).all()) for t in leaves)
    return out, raw, uni


@needs_reference
@pytest.mark.parametrize("case", list(fref.FLOW_BLOCK_CASES))
def test_reference_flow_loss_unchanged(backend, case):
    """``FlowLoss`` (app/loss/flow.py, loaded unchanged) over two classes' ``raw_per_obj_model`` / ``uniform_samples``: the keys, their
    order and the values of ``losses.flow_block_terms`` -- a constant w, an annealed w (``get_anneal_val`` is this package's
    schedule: the glue's stand-in is None), per-term, per-class and module render ratios, an ``empty`` buffer, which is skipped --
    and the committed fixture holds exactly what the reference returns here"""
    sys.path.insert(0, str(FLOW_FIXTURE.parent))
    try:
        import make_flow_loss_fixture as mk
        want = mk.reference_cases()[case]
    finally:
        sys.path.remove(str(FLOW_FIXTURE.parent))
    assert want == json.loads(FLOW_FIXTURE.read_text())[case]
    out, _, _ = _block_run(case, backend)
    _block_check(case, out, want)


@pytest.mark.parametrize("case", list(fref.FLOW_BLOCK_CASES))
def test_flow_block_replayed_from_the_fixture(backend, case):
    """the same comparison against the reference's recorded values, where the reference is absent; which inputs get a gradient"""
    want = json.loads(FLOW_FIXTURE.read_text())[case]
    out, raw, uni = _block_run(case, backend)
    _block_check(case, out, want)
    assert raw["dyn0"]["volume_buffer"]["flow_fwd_pred_bwd"].grad is not None
    block, _ = fref.FLOW_BLOCK_CASES[case]
    assert (uni["Dynamic"]["flow_bwd_pred_fwd"].grad is not None) == bool(block.get("on_uniform_samples", True))


def test_flow_block_keys_and_refusals(backend):
    """the yaml's block gives the four keys of the class; a term without w and anneal, and uniform samples without the class or a
    flow key, are refused by name"""
    from neuralsim_amd import losses
    raw, uni = fref.flow_block_inputs(torch.float32, backend)
    out = losses.flow_block_terms(fref.YAML_FLOW_BLOCK, raw, uni, 0)
    assert list(out) == ["loss_flow_cycle.Dynamic.uniform", "loss_flow_sparsity.Dynamic.uniform", "loss_flow_cycle.Dynamic.render",
                         "loss_flow_sparsity.Dynamic.render"]
    with pytest.raises(ValueError, match="cycle"):
        losses.flow_block_terms(dict(class_name_cfgs=dict(Dynamic=dict(cycle=dict(on_render_ratio=1.0)))), raw, uni, 0)
    with pytest.raises(ValueError, match="Dynamic"):
        losses.flow_block_terms(fref.YAML_FLOW_BLOCK, raw, dict(Pedestrian=uni["Pedestrian"]), 0)
    short = dict(Dynamic={k: v for k, v in uni["Dynamic"].items() if k != "flow_bwd"})
    with pytest.raises(ValueError, match="flow_bwd"):
        losses.flow_block_terms(fref.YAML_FLOW_BLOCK, raw, short, 0)


# ------------------------------------------------------------------------------------------------ 3. the with-flow model
import dynamic_nerf_ref as dr      # noqa: E402
import test_dynamic_nerf as tdn    # noqa: E402  (the scene, the marcher and the yaml block of the model without flow)

RES = (8, 4, 4)


def flow_yaml_params(L_dyn=6, L_flow=16, log2T=10, n_appear=0, dtype="float", **over):
    """the ``Dynamic`` block of fg_emernerf/no_gtbox_with_flow.240208.yaml with the sizes overridden down"""
    fe = dict(type="permuto", param=dict(permuto_auto_compute_cfg=dict(
        type="multi_res", coarsest_res=4.0, finest_res=32.0, n_levels=L_flow, n_feats=2, log2_hashmap_size=log2T,
        apply_random_shifts_per_level=True)))
    kw = dict(use_flow_field=True, use_flow_in_obj=True, flow_encoding_cfg=fe, flow_decoder_cfg=dict(type="mlp", D=2, W=64))
    kw.update(over)
    return tdn.yaml_params(L_dyn, log2T, n_appear, dtype=dtype, res=RES, **kw)


def build_flow(backend, L_dyn=6, L_flow=16, log2T=10, n_appear=0, precision="f32", T=5, seed=11):
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    m = EmerNeRFOnlyDynamicModel(**flow_yaml_params(L_dyn, L_flow, log2T, n_appear, {"f32": "float", "fp16": "half"}[precision]))
    ts = tdn.keyframes(T)
    m.populate(aabb=tdn.AABB, ts_keyframes=ts, accel_n_jump_frames=2)
    p = dr.make_dyn_params(ts, tdn.AABB, L_dyn, log2T, 4.0, 32.0, n_appear, seed=seed)
    fp = fref.make_flow_params(L_flow, log2T, seed=seed + 6)
    assert torch.equal(m.flow_encoding.cfg.permuto.shifts, fp.spec.shifts) and fp.spec.n_params == m.flow_encoding.cfg.n_params
    assert not torch.equal(m.flow_encoding.cfg.permuto.shifts[:1], m.encoding.cfg.permuto.shifts[:1])     # its own shifts
    with torch.no_grad():
        m.encoding.flattened_params.copy_(p.grid.float())
        m.den_w.copy_(torch.cat([w.reshape(-1) for w in p.den_w]).float())
        m.den_b.copy_(torch.cat(p.den_b).float())
        m.rad_w.copy_(torch.cat([w.reshape(-1) for w in p.rad_w]).float())
        m.rad_b.copy_(torch.cat(p.rad_b).float())
        m.flow_encoding.flattened_params.copy_(fp.grid.float())
        m.flow_w.copy_(fp.w.float())
        m.flow_b.copy_(fp.b.float())
    m = m.to(backend)
    occ = tdn.pattern(m.accel.K, RES)
    m.accel.occ_val.copy_(occ.float().reshape(-1).to(backend))
    m.accel.pack_bits()
    return m, p, fp, occ


_SAMPLES = {}


def marched_samples(S, T):
    """the first S samples the restated marcher emits on the rays of tests/test_dynamic_nerf.py (hand-set occupancy); the rays'
    times run over the first and the last keyframe (both clamps of w+-), a midpoint, an off-grid value and both sides outside"""
    if (S, T) not in _SAMPLES:
        R = 64
        r = dict(tdn.rays(R))
        kf = tdn.keyframes(T)
        cand = torch.stack([kf[0], kf[-1], (kf[0] + kf[-1]) * 0.5, kf[0] - 0.5, kf[-1] + 0.75, kf[0] + 0.0625])
        r["ts"] = cand[torch.arange(R) % 6]
        hit = r["hit"]
        K = len(kf[::2])
        occ = tdn.pattern(K, RES)
        sl = dr.slice_of(kf[::2], r["ts"][hit])
        t, ridx, _, _ = dr.march_sliced(r["o"][hit], r["d"][hit], r["near"][hit], r["far"][hit], torch.zeros(int(hit.sum())), sl, occ,
                                        tdn.AABB, list(RES), tdn.STEP, tdn.MAX_STEPS)
        assert t.shape[0] >= S, t.shape
        t, ridx = t[:S], ridx[:S]
        o, d = r["o"][hit], r["d"][hit]
        g = torch.Generator().manual_seed(S + T)
        _SAMPLES[(S, T)] = dict(x=(o[ridx] + t[:, None] * d[ridx]).float(), ridx=ridx, d=d, ts=r["ts"][hit], ha=r["ha"][hit],
                                ws=torch.randn(S, generator=g) * 0.1, wa=torch.randn(S, generator=g), wr=torch.randn(S, 3, generator=g))
    return _SAMPLES[(S, T)]


def flow_query(m, backend, q, ha=None, with_rgb=True):
    dv = lambda t: t.to(backend).contiguous()      # noqa: E731
    S = q["x"].shape[0]
    w = m.time_coord(dv(q["ts"][q["ridx"]]))
    x4 = m._points(w, S, x=dv(q["x"]))
    return m._query(ha, x4, dv(q["d"]), dv(q["ridx"]), tdn.STEP, with_rgb)


W_CYCLE, W_SPARSITY = 1.0, 0.1
# fp16 cannot hold 6.24e-2 on the FLOW TABLE's gradient: it is the scatter of dh_f = W1^T d a1, a 64-term sum that nearly cancels when
# the flow lattice has few features (L_flow = 1: two), and d a1 enters the MFMA with 11 bits.  Measured against the float64
# restatement over FLOW_PARITY x seeds 11, 12, 13, the same on the emulator and on the MI355X: worst 2.436e-1 (the colour term alone,
# S = 33, T = 5, L 16 / 1, seed 13; 1.654e-1 for the whole loss there; every other case <= 9.9e-2).  The constant is twice the worst
# value: the seed-to-seed spread of fp16 rounding through one more hidden layer.  flow_w / flow_b (worst 5.52e-2 / 5.40e-2), every
# other gradient and every f32 bound stay on the family's.
FLOW_GRAD_TOL_FP16 = 4.88e-1
# (S, T, n_appear, L_dyn, L_flow): every S, T and appearance width, both level pairs
FLOW_PARITY = [(1, 5, 0, 6, 16), (31, 2, 4, 6, 16), (32, 1, 0, 16, 1), (33, 5, 4, 16, 1), (257, 5, 4, 6, 16), (257, 1, 4, 16, 1),
               (257, 2, 0, 6, 16), (33, 2, 0, 16, 1)]


def flow_parity_errors(backend, precision, S, T, n_appear, L_dyn, L_flow, seed=11):
    """-> (value errors, gradient errors) of the with-flow query against the float64 restatement"""
    from neuralsim_amd import losses
    m, p, fp, _ = build_flow(backend, L_dyn, L_flow, 10, n_appear, precision, T, seed=seed)
    q = marched_samples(S, T)
    for t in p.tensors() + fp.tensors():
        t.requires_grad_(True)
    ha64 = leaf(q["ha"], dtype=torch.float64) if n_appear else None
    ref = fref.query_points(p, fp, q["x"], q["ts"][q["ridx"]], q["d"][q["ridx"]], ha64[q["ridx"]] if n_appear else None, tdn.STEP)
    colour64 = (ref["rgb"] * q["wr"].double()).sum() + (ref["sigma"] * q["ws"].double()).sum() + \
        (ref["opacity_alpha"] * q["wa"].double()).sum()
    (gflow_colour,) = torch.autograd.grad(colour64, fp.grid, retain_graph=True)
    cyc64, spa64 = fref.flow_loss(*[ref[k] for k in fref.FLOW_KEYS], w_cycle=W_CYCLE, w_sparsity=W_SPARSITY)
    (colour64 + cyc64 + spa64).backward()
    refg = dict(tdn.flat_grads(p), flow_grid=fp.grid.grad, flow_w=fp.w.grad, flow_b=fp.b.grad)
    if n_appear:
        refg["h_appear"] = ha64.grad
    ha = leaf(q["ha"], backend) if n_appear else None
    sigma, alpha, rgb, flow = flow_query(m, backend, q, ha)
    colour = (rgb * q["wr"].to(backend)).sum() + (sigma * q["ws"].to(backend)).sum() + (alpha * q["wa"].to(backend)).sum()
    (gc,) = torch.autograd.grad(colour, m.flow_encoding.flattened_params, retain_graph=True)
    cyc, spa = losses.flow_loss(*[flow[k] for k in fref.FLOW_KEYS], w_cycle=W_CYCLE, w_sparsity=W_SPARSITY)
    (colour + cyc + spa).backward()
    sync(backend)
    ev = dict(sigma=float((sigma.detach().cpu() - ref["sigma"].detach()).abs().max()) / (1 + float(ref["sigma"].detach().max())),
              alpha=float((alpha.detach().cpu() - ref["opacity_alpha"].detach()).abs().max()) / 10,
              rgb=float((rgb.detach().cpu() - ref["rgb"].detach()).abs().max()))
    for k in fref.FLOW_KEYS:
        assert flow[k].shape == (S, 3) and flow[k].dtype == torch.float32
        ev[k] = float((flow[k].detach().cpu() - ref[k].detach()).abs().max()) / (1 + float(ref[k].detach().abs().max()))
    print(f"[flow model {precision} S={S} T={T} na={n_appear} L={L_dyn}/{L_flow}] values", {k: f"{v:.2e}" for k, v in ev.items()})
    got = dict(grid=m.encoding.flattened_params.grad, den_w=m.den_w.grad, den_b=m.den_b.grad, rad_w=m.rad_w.grad, rad_b=m.rad_b.grad,
               flow_grid=m.flow_encoding.flattened_params.grad, flow_w=m.flow_w.grad, flow_b=m.flow_b.grad)
    if n_appear:
        got["h_appear"] = ha.grad
    eg = {k: rel_l2(got[k].cpu(), refg[k]) for k in refg}
    eg["flow_grid(colour)"] = rel_l2(gc.cpu(), gflow_colour)
    print("    gradients", {k: f"{v:.2e}" for k, v in eg.items()})
    assert float(gflow_colour.abs().max()) > 0 and float(gc.abs().max()) > 0
    return ev, eg


FLOW_PARAM_GRADS = ("flow_grid", "flow_grid(colour)")          # the quantities FLOW_GRAD_TOL_FP16 is for


@pytest.mark.parametrize("S,T,n_appear,L_dyn,L_flow", FLOW_PARITY)
@pytest.mark.parametrize("precision", ["f32", "fp16"])
def test_flow_model_parity(backend, precision, S, T, n_appear, L_dyn, L_flow):
    """sigma / alpha / rgb, the four flow tensors and every gradient -- both tables, both decoders, the radiance decoder, the
    appearance codes -- of a loss made of a colour term, the cycle term and the sparsity term, against the float64 restatement;
    the flow table gets a gradient from the colour term alone (through the warped positions)"""
    ev, eg = flow_parity_errors(backend, precision, S, T, n_appear, L_dyn, L_flow)
    for k, e in ev.items():
        assert e < VAL_TOL[precision], (k, e)
    for k, e in eg.items():
        tol = FLOW_GRAD_TOL_FP16 if (precision == "fp16" and k in FLOW_PARAM_GRADS) else GRAD_TOL[precision]
        assert e < tol, (k, e, tol)


# ------------------------------------------------------------------------------------------------ 4. aggregation identity
def test_aggregation_identity(backend):
    """a flow decoder whose last layer is zero and one keyframe (delta = 0): the three plane sets coincide, so sigma / rgb are those
    of the model without flow on the same dynamic weights -- within the f32 value bound, not bit for bit (the blend rounds)"""
    m, p, _, _ = build_flow(backend, 6, 16, 10, 4, "f32", T=1)
    with torch.no_grad():
        F = m.flow_encoding.cfg.out_features
        m.flow_w[64 * F + 4096:] = 0.0
        m.flow_b[128:] = 0.0
    m0, _, _ = tdn.build(backend, 6, 10, 4, "f32", T=1)
    q = marched_samples(257, 1)
    ha = q["ha"].to(backend)
    with torch.no_grad():
        sigma, alpha, rgb, flow = flow_query(m, backend, q, ha)
        s0, a0, rgb0 = tdn.decode(m0, backend, q, ha)
    assert all(not bool(flow[k].any()) for k in fref.FLOW_KEYS)
    assert float((sigma - s0).abs().max()) < VAL_TOL["f32"] * (1 + float(s0.max()))
    assert float((rgb - rgb0).abs().max()) < VAL_TOL["f32"] and float((alpha - a0).abs().max()) < 10 * VAL_TOL["f32"]


# ------------------------------------------------------------------------------------------------ 5. flow off
def test_no_flow_model_has_no_flow_parts(backend):
    """the yaml block without flow: no flow parameter in the state dict, no flow key in the volume buffer or the uniform samples"""
    m, _, _ = tdn.build(backend)
    assert not m.use_flow and not any("flow" in k for k in m.state_dict())
    assert [g["name"] for g in m._param_groups({})] == ["encoding", "dynamic_decoder", "radiance_decoder"]
    _, ret = tdn.run_query(m, backend, 16)
    assert ret["volume_buffer"]["type"] == "packed" and not any("flow" in k for k in ret["volume_buffer"])
    assert not any("flow" in k for k in m.sample_pts_uniform(8))


# ------------------------------------------------------------------------------------------------ 8. config, outputs, state
FLOW_GOLDEN = Path(__file__).resolve().parent / "golden" / "emernerf_flow_model_params.yaml"
FLOW_REF_YAML = ref_glue.REF_ROOT / "code_multi" / "configs" / "exps" / "fg_emernerf" / "no_gtbox_with_flow.240208.yaml"


def _golden_params():
    import yaml
    return yaml.safe_load(FLOW_GOLDEN.read_text())


def _shrunk(p):
    """the committed block with the sizes overridden down"""
    import copy
    p = copy.deepcopy(p)
    for k in ("dynamic_encoding_cfg", "flow_encoding_cfg"):
        p[k]["param"]["permuto_auto_compute_cfg"].update(n_levels=4, log2_hashmap_size=8, coarsest_res=4.0, finest_res=32.0)
    p["accel_cfg"] = dict(p["accel_cfg"], resolution=list(RES))
    p["accel_cfg"].pop("vox_size", None)
    p["ray_query_cfg"] = dict(query_mode="march_occ", query_param=dict(march_cfg=dict(step_size=tdn.STEP, max_steps=tdn.MAX_STEPS)))
    return p


def test_flow_yaml_block_builds_and_queries(backend):
    """the ``Dynamic`` model_params of no_gtbox_with_flow.240208.yaml (committed as a settings-only fixture; compared with the
    reference's file where it is readable) builds with the sizes overridden down; ``ray_query`` and ``sample_pts_uniform`` carry
    the four flow keys; the optimiser sees the flow table and decoder, the weight regulariser the flow weights; a state_dict round
    trip into a fresh model reproduces the query bit for bit; the level mask touches the dynamic lattice only"""
    from neuralsim_amd.fields.dynamic_nerf import EmerNeRFOnlyDynamicModel
    params = _golden_params()
    if ref_glue.readable(FLOW_REF_YAML):
        from nr3d_lib.config import load_config
        ref = load_config(str(FLOW_REF_YAML))["assetbank_cfg"]["Dynamic"]["model_params"]
        assert (ref.to_dict() if hasattr(ref, "to_dict") else dict(ref)) == params
    assert params["use_flow_field"] is True and params["flow_decoder_cfg"] == dict(type="mlp", D=2, W=64)
    small = _shrunk(params)
    torch.manual_seed(0)
    m = EmerNeRFOnlyDynamicModel(**small).populate(aabb=tdn.AABB, ts_keyframes=tdn.keyframes(5), device=backend)
    with torch.no_grad():       # (the tables start at 1e-4: give the flow something to say)
        m.flow_encoding.flattened_params.mul_(3000.0)
        m.encoding.flattened_params.mul_(3000.0)
    assert m.use_flow and [g["name"] for g in m._param_groups({})] == ["encoding", "dynamic_decoder", "radiance_decoder",
                                                                       "flow_encoding", "flow_decoder"]
    assert any(t is m.flow_w for t in m._weight_reg_tensors())
    sd = m.state_dict()
    assert {"flow_encoding.flattened_params", "flow_w", "flow_b"} <= set(sd)
    r = tdn.rays(16)
    ha = (r["ha"] if m.n_appear else None)
    tested, ret = tdn.run_query(m, backend, 16, ha=None if ha is None else ha.to(backend))
    vb = ret["volume_buffer"]
    S = vb["t"].shape[0]
    assert S > 0 and all(vb[k].shape == (S, 3) and vb[k].dtype == torch.float32 for k in fref.FLOW_KEYS)
    assert float(vb["flow_fwd"].detach().abs().max()) > 0
    uni = m.sample_pts_uniform(33, generator=torch.Generator(device=backend).manual_seed(1))
    assert all(uni[k].shape == (33, 3) for k in fref.FLOW_KEYS) and uni["sigma"].shape == (33,)
    m2 = EmerNeRFOnlyDynamicModel(**small).populate(aabb=tdn.AABB, ts_keyframes=tdn.keyframes(5), device=backend)
    m2.load_state_dict(sd)
    _, ret2 = tdn.run_query(m2, backend, 16, ha=None if ha is None else ha.to(backend))
    for k in ("sigma", "rgb", "opacity_alpha") + fref.FLOW_KEYS:
        assert torch.equal(ret2["volume_buffer"][k], vb[k]), k
    m.set_active_levels(2)
    assert m.encoding.cfg.pmeta.n_active_levels == 2 and m.flow_encoding.cfg.pmeta.n_active_levels == 0
    m.set_active_levels(None)
    # query_density (the occupancy refresh, collect) is the aggregated density the renderer sees
    with torch.no_grad():
        x = (tested["rays_o"][vb["rays_inds_hit"].new_zeros(1)] * 0 + torch.tensor([[0.3, 0.2, -0.1]], device=backend))
        ts = tdn.keyframes(5)[1:2].to(backend)
        assert torch.equal(m.query_density(x, ts), m.forward_density(x, ts)["sigma"])


@pytest.mark.parametrize("key,over", [
    ("use_flow_in_obj", dict(use_flow_in_obj=False)),
    ("flow_decoder_cfg.D", dict(flow_decoder_cfg=dict(type="mlp", D=3, W=64))),
    ("flow_decoder_cfg.W", dict(flow_decoder_cfg=dict(type="mlp", D=2, W=128))),
    ("flow_decoder_cfg.output_activation", dict(flow_decoder_cfg=dict(type="mlp", D=2, W=64, output_activation="tanh"))),
    ("flow_decoder_cfg.last_bias", dict(flow_decoder_cfg=dict(type="mlp", D=2, W=64, last_bias=False))),
    ("n_feats", dict(flow_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=dict(type="multi_res", n_feats=4))))),
    ("n_levels", dict(flow_encoding_cfg=dict(type="permuto", param=dict(permuto_auto_compute_cfg=dict(type="multi_res", n_levels=17))))),
    ("flow_encoding_cfg.type", dict(flow_encoding_cfg=dict(type="lotd"))),
    ("use_flow_field", dict(flow_encoding_cfg=None)),
    ("use_flow_field", dict(flow_decoder_cfg=None)),
])
def test_flow_refused_options(key, over):
    from neuralsim_amd.fields import ref_config
    import re
    with pytest.raises(NotImplementedError, match=re.escape(key)):
        ref_config.validate_emernerf_params(flow_yaml_params(**over))


# ------------------------------------------------------------------------------------------------ 9. training steps in a compose
def test_flow_compose_training_steps(backend):
    """a few Adam steps of a compose render -- a static street NeuS plus this model as ``Dynamic`` -- with the yaml's ``flow`` block on:
    the per-object volume buffer reaches the loss with its four flow keys intact, all four flow terms appear and are finite, every
    parameter group of the model (the flow table and decoder included) moves in a step, and the occupancy refresh runs on the
    aggregated density"""
    from neuralsim_amd import losses
    from neuralsim_amd.fields.neus import OccGridAccel
    from neuralsim_amd.renderers.buffer_compose_renderer import BufferComposeRenderer, Drawable
    from util import make_params, model_from_params
    box = torch.tensor([[-1.0, -1, -1], [1.0, 1, 1]])
    pm = make_params(sdf_D=2, small=True, sphere=True, seed=11, ln_inv_s=0.45, grid_bound=2e-2, noise_scale=1.0)
    street = model_from_params(pm, backend, precision="f32")
    street.accel = OccGridAccel(box, resolution=[8, 8, 8], device=backend)
    street.accel.set_all_occupied()
    street.ray_query_cfg = dict(query_mode="march_occ_multi_upsample",
                                query_param=dict(num_coarse=8, num_fine=[4, 4], upsample_inv_s=64.0, upsample_inv_s_factors=[1, 4],
                                                 march_cfg=dict(step_size=0.05, max_steps=128)))
    dyn, _, _, _ = build_flow(backend, 4, 4, 8, 4, "f32", T=5)
    R = 24
    r = tdn.rays(70)
    dv = lambda a: a[:R].to(backend).contiguous()      # noqa: E731
    o = r["o"] * torch.tensor([0.6, 1.0, 1.0])
    gt = torch.rand(R, 3, generator=torch.Generator().manual_seed(2)).to(backend)
    rend = BufferComposeRenderer(dict(with_rgb=True, with_normal=False, near=0.01, depth_use_normalized_vw=True)).train()
    drawables = [Drawable("street", "Street", street), Drawable("dyn", "Dynamic", dyn)]
    opt = dyn.training_setup(dict(lr=1e-2, eps=1e-15, betas=[0.9, 0.99]))
    dyn.training_initialize()
    dyn.accel.n_steps_warmup, dyn.accel.n_steps_between_update = 2, 2       # the refresh runs at it = 2
    dyn.refresh_generator = torch.Generator(device=backend).manual_seed(3)
    names = [g["name"] for g in opt.param_groups]
    assert "flow_encoding" in names and "flow_decoder" in names
    keys = ["loss_flow_cycle.Dynamic.uniform", "loss_flow_sparsity.Dynamic.uniform", "loss_flow_cycle.Dynamic.render",
            "loss_flow_sparsity.Dynamic.render"]
    fracs = []
    for it in range(4):
        dyn.training_before_per_step(it)
        fracs.append(dyn.accel.frac_occupied(per_slice=True).cpu())
        before = [[p.detach().clone() for p in g["params"]] for g in opt.param_groups]
        ret = rend(dv(o), dv(r["d"]), drawables=drawables, rays_h_appear=dv(r["ha"]), rays_ts=dv(r["ts"]), return_buffer=True,
                   return_details=True, bypass_ray_query_cfg=dict(Street=dict(perturb=False), Dynamic=dict(perturb=False)))
        raw = ret["raw_per_obj_model"]
        assert raw["dyn"]["class_name"] == "Dynamic" and all(k in raw["dyn"]["volume_buffer"] for k in fref.FLOW_KEYS)
        uni = dict(Dynamic=dyn.sample_pts_uniform(64, generator=torch.Generator(device=backend).manual_seed(it)))
        terms = losses.flow_block_terms(fref.YAML_FLOW_BLOCK, raw, uni, it)
        assert list(terms) == keys and all(bool(torch.isfinite(v)) for v in terms.values())
        loss = ((ret["rendered"]["rgb_volume"] - gt) ** 2).mean() + sum(terms.values()) + 1e-3 * uni["Dynamic"]["sigma"].mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        dyn.training_after_per_step(it)
        for g, old in zip(opt.param_groups, before):
            assert any(not torch.equal(p.detach(), q) for p, q in zip(g["params"], old)), g["name"]
    assert bool((fracs[1] == 1.0).all()) and float(dyn.accel.occ_val.max()) > 1.0e-2 and not torch.equal(fracs[3], fracs[1])
    assert all(bool(torch.isfinite(p).all()) for p in dyn.parameters())
