"""The 16-point backward of the SDF branch (k_field_bwd_h: fp16, <= 16 levels, no embedded block) against the 32-point
kernel it replaces (``NSIM_BWD_TILE=32``, read per launch) and against the oracle."""
import pytest
import torch

from oracle import field as ofield
from neuralsim_amd import _lib
from neuralsim_amd.fields.neus import _FieldFn
from util import SMALL_RES as SMALL_RES_T, leaf, make_params, model_from_params, oracle_flat_grads, rel_l2


def _tile(monkeypatch, tile):
    if tile == 32:
        monkeypatch.setenv("NSIM_BWD_TILE", "32")
    else:
        monkeypatch.delenv("NSIM_BWD_TILE", raising=False)


def _direct(model, backend, S, seed, n_dead=0):
    """nsim_field_bwd_sdf on random planes; rows past S (up to the pitch) hold NaN, which no output may see.
    -> (dsdf_w, dsdf_b, dh planes, g planes, dL/dx) on the CPU"""
    g = torch.Generator().manual_seed(seed)
    PS = max(32, (S + 31) // 32 * 32)
    NL = model.field_meta.lotd.num_levels
    h = torch.randn(16, PS, 2, generator=g) * 0.5
    J = torch.randn(16, PS, 6, generator=g) * 0.5
    h[NL - n_dead:], J[NL - n_dead:] = 0.0, 0.0          # levels past num_levels / masked: zeros, as the gather writes them
    h[:, S:], J[:, S:] = float("nan"), float("nan")
    gs = torch.randn(S, generator=g)
    gn = torch.randn(S, 3, generator=g) * 0.3
    dv = lambda a: a.to(backend).contiguous()
    out = dict(w=torch.zeros_like(model.sdf_w.detach()), b=torch.zeros_like(model.sdf_b.detach()),
               dh=dv(torch.zeros(16, max(S, 1), 2)), g=dv(torch.zeros(16, max(S, 1), 2)), dx=dv(torch.zeros(max(S, 1), 3)))
    _lib.call("nsim_field_bwd_sdf", model.field_meta, _lib.ptr(model._weight_pack()), _lib.ptr(dv(h)), _lib.ptr(dv(J.half())), S,
              _lib.ptr(dv(gs)), _lib.ptr(dv(gn)), _lib.ptr(out["dh"]), _lib.ptr(out["g"]), _lib.ptr(out["w"]), _lib.ptr(out["b"]),
              _lib.ptr(out["dx"]), PS)
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("sdf_D", [1, 2])
@pytest.mark.parametrize("S", [0, 5, 77, 200])
def test_bwd16_equals_bwd32(backend, sdf_D, S, monkeypatch):
    """Every output of the SDF-branch backward -- weight and bias gradients, the dh / g hand-off planes, dL/dx -- of the
    16-point kernel against the 32-point one: S = 0, S < 16, S neither a multiple of 16 nor of 64, several groups."""
    p = make_params(sdf_D=sdf_D, small=True, sphere=False, grid_bound=0.3, seed=7, noise_scale=1.0)
    model = model_from_params(p, backend, precision="fp16")
    assert model.field_meta.lotd.num_levels <= 16
    res = {}
    for tile in (32, 16):
        _tile(monkeypatch, tile)
        res[tile] = _direct(model, backend, S, seed=S + 11)
    a, b = res[32], res[16]
    if S == 0:
        for k in a:
            assert float(b[k].abs().max()) == 0.0, k
        return
    assert not torch.equal(b["w"], a["w"])      # two kernels: the knob switched (accumulation orders differ)
    for k in ("w", "b"):
        assert bool(torch.isfinite(b[k]).all()) and float(b[k].abs().max()) > 0, k
        assert rel_l2(b[k], a[k]) < 1e-2, (k, rel_l2(b[k], a[k]))
    NL = model.field_meta.lotd.num_levels
    for k in ("dh", "g"):
        x, y = b[k][:NL, :S], a[k][:NL, :S]
        assert bool(torch.isfinite(x).all()), k
        assert (x - y).abs().max() < 4e-3 * (1 + y.abs().max()), (k, float((x - y).abs().max()))
    assert bool(torch.isfinite(b["dx"][:S]).all())
    assert rel_l2(b["dx"][:S], a["dx"][:S]) < 1e-2


@pytest.mark.parametrize("sdf_D", [1, 2])
@pytest.mark.parametrize("S", [9, 77, 150])
def test_bwd16_against_the_oracle(backend, sdf_D, S):
    """The fp16 with-grad query end to end (its SDF-branch backward on the 16-point kernel): every gradient against the
    oracle at the tolerances of tests/test_field.py's fp16 cases."""
    p = make_params(sdf_D=sdf_D, small=True, sphere=False, grid_bound=0.3, seed=5, noise_scale=1.0)
    for t in p.tensors():
        t.requires_grad_(True)
    model = model_from_params(p, backend, precision="fp16")
    g = torch.Generator().manual_seed(3 + S)
    R = 7
    rays_o = torch.randn(R, 3, generator=g) * 0.1
    rays_d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    ridx = torch.randint(0, R, (S,), generator=g).sort().values
    t = torch.rand(S, generator=g) * 0.8
    h_appear = torch.randn(R, 4, generator=g) * 0.5
    x = rays_o[ridx] + t[:, None] * rays_d[ridx]
    sdf_r, nab_r, rgb_r = ofield.forward_field(x, rays_d[ridx], leaf(h_appear)[ridx], p)
    dv = lambda a: a.to(backend).contiguous()
    sdf, nab, rgb = _FieldFn.apply(model, model.encoding.flattened_params, model.sdf_w, model.sdf_b, model.rad_w,
                                   model.rad_b, leaf(h_appear, backend), None, dv(rays_o), dv(rays_d), dv(t), dv(ridx), True)
    ws, wn, wr = torch.randn(S, generator=g), torch.randn(S, 3, generator=g) * 0.1, torch.randn(S, 3, generator=g)
    (sdf_r * ws).sum().add((nab_r * wn).sum()).add((rgb_r * wr).sum()).backward()
    (sdf * dv(ws)).sum().add((nab * dv(wn)).sum()).add((rgb * dv(wr)).sum()).backward()
    ref = oracle_flat_grads(p)
    got = dict(grid=model.encoding.flattened_params.grad, sdf_w=model.sdf_w.grad, sdf_b=model.sdf_b.grad)
    for k, v in got.items():
        e = rel_l2(v.cpu(), ref[k])
        assert e < 3e-2, (k, e)


def test_bwd16_hardmask(backend, monkeypatch):
    """Hardmask level annealing (n_active < num_levels) in fp16 mode: the 16-point kernel's gradients against the oracle
    and against the 32-point kernel; the masked levels get exactly zero gradient."""
    n_active = 9
    p = ofield.make_field_params(lod_res=list(SMALL_RES_T), log2_hashmap_size=12, sdf_D=2, seed=5, sphere_init=False,
                                 grid_bound=0.3, noise_scale=1.0)
    p.grid = p.grid.float()
    p.spec.n_active = n_active
    g = torch.Generator().manual_seed(2)
    R, S = 5, 90
    rays_o = torch.randn(R, 3, generator=g) * 0.1
    rays_d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    ridx = torch.randint(0, R, (S,), generator=g).sort().values
    t = torch.rand(S, generator=g) * 0.8
    h_appear = torch.randn(R, 4, generator=g) * 0.5
    ws, wn, wr = torch.randn(S, generator=g), torch.randn(S, 3, generator=g) * 0.1, torch.randn(S, 3, generator=g)
    dv = lambda a: a.to(backend).contiguous()
    grads = {}
    for tile in (32, 16):
        _tile(monkeypatch, tile)
        for q in p.tensors():
            q.grad = None
            q.requires_grad_(True)
        model = model_from_params(p, backend, precision="fp16")
        model.set_active_levels(n_active)
        sdf, nab, rgb = _FieldFn.apply(model, model.encoding.flattened_params, model.sdf_w, model.sdf_b, model.rad_w,
                                       model.rad_b, leaf(h_appear, backend), None, dv(rays_o), dv(rays_d), dv(t), dv(ridx), True)
        (sdf * dv(ws)).sum().add((nab * dv(wn)).sum()).add((rgb * dv(wr)).sum()).backward()
        grads[tile] = dict(grid=model.encoding.flattened_params.grad.cpu(), sdf_w=model.sdf_w.grad.cpu(),
                           sdf_b=model.sdf_b.grad.cpu())
    x = rays_o[ridx] + t[:, None] * rays_d[ridx]
    sdf_r, nab_r, rgb_r = ofield.forward_field(x, rays_d[ridx], leaf(h_appear)[ridx], p)
    (sdf_r * ws).sum().add((nab_r * wn).sum()).add((rgb_r * wr).sum()).backward()
    ref = oracle_flat_grads(p)
    off = p.spec.lod_offsets[n_active]
    for k, v in grads[16].items():
        assert rel_l2(v, ref[k]) < 3e-2, (k, rel_l2(v, ref[k]))
        assert rel_l2(v, grads[32][k]) < 1e-2, (k, rel_l2(v, grads[32][k]))
    assert float(grads[16]["grid"][off:].abs().max()) == 0.0
    assert float(grads[16]["grid"][:off].abs().max()) > 0.0
