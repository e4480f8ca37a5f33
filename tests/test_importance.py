"""Error-map importance sampling of training pixels (neuralsim_amd/importance.py on the ``nsim_errmap_*`` kernels)
against the float64 restatement tests/importance_ref.py, and its wiring into RenderTrainer.

Bounds (u = 2^-24, the unit roundoff of f32; M = max(max |val|, max |em_old|)):
  update   |em - ref| <= (c + 3) u M for a cell hit c times: the c-term f32 sum in any order is off by at most (c - 1) u c M, c u M
           after the division by c; the division, the two halvings (exact) and the sum of the blend add at most 3 u M.
           The pred / gt form computes the per-ray error in f32: one rounding per difference (two once squared), the square, two
           sums and the division by 3 -- at most 7 u relative per ray, entering the map halved: (c + 3 + 4) u M.
           A second call on the same object: the error of the first enters halved, err2 <= err1 / 2 + (c2 + 3) u M.
  CDF      h w u against the float64 CDF (the serial-sum bound for terms summing to 1), n_images u for the image level.
  draw     a row that chose index i for the uniform v satisfies C64[i-1] - eps <= v <= C64[i] + eps with the eps of that CDF."""
import importlib

import pytest
import torch

import importance_ref as ref
from conftest import sync
from neuralsim_amd.importance import ErrorMap, ImpSampler

U = 2.0 ** -24


def _maps(V, hw, backend, seed=0, kind="random", **kw):
    """an ErrorMap on the backend's device carrying a non-trivial map (f32 values, returned as well)"""
    g = torch.Generator().manual_seed(seed)
    h, w = hw
    if kind == "ones":
        em0 = torch.ones([V, h, w])
    else:
        em0 = torch.rand([V, h, w], generator=g) ** 3 * 2.0 + 0.01
        if kind == "zeros":                       # exact zeros: the lower clamp of the pdf is active
            em0[torch.rand([V, h, w], generator=g) < 0.4] = 0.0
            em0[-1] = 1.0                           # ... next to an all-ones image
    em = ErrorMap(V, error_map_hw=hw, device=backend, **kw)
    with torch.no_grad():
        em.error_map.copy_(em0.to(backend))
    em.invalidate()
    return em, em0


def _update_case(case, seed=0):
    g = torch.Generator().manual_seed(seed)
    if case == "a":       # many collisions per cell, image 1 never hit, pixels on the clamps and exactly on cell borders
        V, hw, N = 3, (4, 8), 257
        fidx = torch.randint(0, 2, [N], generator=g) * 2
        xy = torch.rand([N, 2], generator=g)
        k = torch.arange(40)
        xy[:40, 0], xy[:40, 1] = (k % 9) / 8.0, (k % 5) / 4.0
        xy[40:44] = torch.tensor([[1e-6, 1e-6], [1 - 1e-6, 1 - 1e-6], [1e-6, 1 - 1e-6], [0.0, 1.0]])
    else:
        V, hw, N = 5, (32, 64), 8192
        fidx = torch.randint(0, V, [N], generator=g)
        xy = torch.rand([N, 2], generator=g).clamp_(1e-6, 1 - 1e-6)
    val = torch.rand([N], generator=g) ** 2 * 3.0
    val2 = torch.rand([N], generator=g) * 0.5
    return V, hw, fidx, xy, val, val2


def _check_update(em_dev, em_ref, cnt, em_old, M, extra=0.0, prev_err=None):
    d = (em_dev.detach().cpu().double() - em_ref).abs()
    hit = cnt > 0
    bound = (cnt.double() + 3 + extra) * U * M + (0.5 * prev_err if prev_err is not None else 0.0)
    worst = float((d[hit] / bound[hit]).max())
    print(f"update: worst error / bound over {int(hit.sum())} hit cells = {worst:.3f}")
    assert bool((d[hit] <= bound[hit]).all()), worst
    assert torch.equal(em_dev.detach().cpu()[~hit], em_old[~hit])          # untouched cells keep their bits
    return bound


@pytest.mark.parametrize("case", ["a", "b"])
def test_update_matches_float64(backend, case):
    V, hw, fidx, xy, val, val2 = _update_case(case)
    em, em0 = _maps(V, hw, backend, seed=1)
    ns0 = em.n_steps.cpu().clone()
    em.step_error_map(fidx.to(backend), xy.to(backend), val.to(backend))
    sync(backend)
    r1, ns1, c1 = ref.update(em0.double(), ns0, fidx, xy, val)
    M1 = max(float(val.max()), float(em0.max()))
    b1 = _check_update(em.error_map, r1, c1, em0, M1)
    assert torch.equal(em.n_steps.cpu(), ns1)
    if case == "a":
        assert int(ns1[1]) == 0 and int(c1[1].sum()) == 0 and int(c1.max()) > 4
    # a second call on the same object: scratch that was not re-zeroed would carry the first call's sums
    em1 = em.error_map.detach().cpu().clone()
    em.step_error_map(fidx.flip(0).to(backend), xy.flip(0).to(backend), val2.to(backend))
    sync(backend)
    r2, ns2, c2 = ref.update(r1, ns1, fidx.flip(0), xy.flip(0), val2)
    M2 = max(float(val2.max()), float(em1.max()))
    _check_update(em.error_map, r2, c2, em1, M2, prev_err=b1)
    assert torch.equal(em.n_steps.cpu(), ns2)
    # ... and against the reference applied to the map the device held after the first call: the bound of one call
    r2d, _, _ = ref.update(em1.double(), ns1, fidx.flip(0), xy.flip(0), val2)
    _check_update(em.error_map, r2d, c2, em1, M2)
    assert float(em._sum.abs().max()) == 0.0 and float(em._cnt.abs().max()) == 0.0 and int(em._touched.abs().max()) == 0


@pytest.mark.parametrize("fn", ["mse", "l1"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_update_from_colours_matches_the_value_form(backend, case, fn):
    V, hw, fidx, xy, _, _ = _update_case(case)
    g = torch.Generator().manual_seed(5)
    pred, gt = torch.rand([fidx.shape[0], 3], generator=g), torch.rand([fidx.shape[0], 3], generator=g)
    e64 = ref.rgb_error(pred, gt, fn)
    em_a, em0 = _maps(V, hw, backend, seed=2)
    em_b, _ = _maps(V, hw, backend, seed=2)
    err = em_a.step_error_map_rgb(fidx.to(backend), xy.to(backend), pred.to(backend), gt.to(backend), fn)
    em_b.step_error_map(fidx.to(backend), xy.to(backend), e64.float().to(backend))
    sync(backend)
    assert err.dtype == torch.float32 and bool(((err.cpu().double() - e64).abs() <= 7 * U * e64).all())
    r, ns, c = ref.update(em0.double(), torch.zeros([V], dtype=torch.long), fidx, xy, e64)
    M = max(float(e64.max()), float(em0.max()))
    _check_update(em_b.error_map, r, c, em0, M)
    _check_update(em_a.error_map, r, c, em0, M, extra=4.0)
    assert torch.equal(em_a.n_steps.cpu(), ns) and torch.equal(em_b.n_steps.cpu(), ns)


def test_single_frame_broadcast_and_state_dict(backend):
    em, em0 = _maps(3, (4, 8), backend, seed=3)
    g = torch.Generator().manual_seed(4)
    xy, val = torch.rand([50, 2], generator=g), torch.rand([50], generator=g)
    em.step_error_map(torch.tensor([2]).to(backend), xy.to(backend), val.to(backend))
    sync(backend)
    r, ns, c = ref.update(em0.double(), torch.zeros([3], dtype=torch.long), torch.tensor([2]), xy, val)
    _check_update(em.error_map, r, c, em0, max(float(val.max()), float(em0.max())))
    assert em.n_steps.cpu().tolist() == [0, 0, 1]
    sd = em.state_dict()
    assert sorted(sd) == ["error_map", "n_steps"]
    em2 = ErrorMap(3, error_map_hw=(4, 8), device=backend)
    em2.load_state_dict(sd)
    assert torch.equal(em2.error_map, em.error_map) and torch.equal(em2.n_steps, em.n_steps)
    assert torch.equal(em2.get_pdf().cpu(), em.get_pdf().cpu())           # the loaded map is what the tables are built from


# ----------------------------------------------------------------------------------------------------------- CDF
@pytest.mark.parametrize("variant", ["zeros_min_pdf", "max_pdf", "ones"])
@pytest.mark.parametrize("hw", [(3, 5), (32, 32), (32, 64), (48, 64)])
def test_cdf_matches_float64(backend, hw, variant):
    V = 4
    kw = dict(zeros_min_pdf=dict(min_pdf=0.01), max_pdf=dict(min_pdf=0.01, max_pdf=4.0), ones=dict(min_pdf=0.01))[variant]
    kind = dict(zeros_min_pdf="zeros", max_pdf="random", ones="ones")[variant]
    em, em0 = _maps(V, hw, backend, seed=7, kind=kind, **kw)
    t = em.tables()
    sync(backend)
    n = hw[0] * hw[1]
    C = t["cdf_cell"].cpu()
    C64 = ref.cdf_cell(em0, kw["min_pdf"], kw.get("max_pdf"))
    assert bool((C[:, 1:] >= C[:, :-1]).all()) and bool((C[:, -1] == 1.0).all()) and bool((C > 0).all())
    d = float((C.double() - C64).abs().max())
    print(f"cdf_cell {hw} {variant}: max |cdf - cdf64| = {d:.3e}, bound {n * U:.3e}")
    assert d <= n * U
    Ci, Ci64 = t["cdf_img"].cpu(), ref.cdf_image(em0)
    assert bool((Ci[1:] >= Ci[:-1]).all()) and float(Ci[-1]) == 1.0
    assert float((Ci.double() - Ci64).abs().max()) <= V * U
    if variant == "zeros_min_pdf":        # the lower clamp is active: zero cells carry min_pdf / (h w) before the last normalisation
        p64 = ref.pdf(em0, 0.01)
        assert float(p64[em0 == 0].min()) > 0.5 * 0.01 / n
    # the public getters against the torch classes on the CPU
    from nr3d_lib.models.importance import TorchErrorMap
    tm = TorchErrorMap(V, error_map_hw=hw, **kw)
    tm.error_map.copy_(em0)
    for a, b in ((em.get_pdf(), tm.get_pdf()), (em.get_pdf([2, 0]), tm.get_pdf([2, 0])), (em.get_pdf_image(), tm.get_pdf_image()),
                 (em.get_normalized_error_map(1), tm.get_normalized_error_map(1))):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert bool(((a.cpu().double() - b.double()).abs() <= 1e-6 * b.double().abs()).all())
    # nothing is rebuilt while the map does not change; an update makes the next reader rebuild, into the other snapshot
    assert em.tables() is t
    em.step_error_map(torch.zeros([1], dtype=torch.long, device=backend), torch.full([1, 2], 0.5, device=backend),
                      torch.full([1], 100.0, device=backend))
    t2 = em.tables()
    assert t2 is not t and t2["cdf_cell"].data_ptr() != t["cdf_cell"].data_ptr() and em.tables() is t2
    assert torch.equal(t["cdf_cell"].cpu(), C)                            # the previous snapshot is left alone


# ----------------------------------------------------------------------------------------------------------- draw
def _stratified(n, g):
    return ((torch.randperm(n, generator=g).double() + 0.5) / n).float()


def _check_rows(fidx, xy, u, em_dev, hw, min_pdf, max_pdf=None, fixed=None):
    """every row: the chosen image / cell brackets its uniform in the float64 CDFs of the map read back from the device"""
    h, w = hw
    V = em_dev.shape[0]
    em0 = em_dev.detach().cpu()
    xy, u = xy.cpu(), u.cpu().double()
    assert xy.dtype == torch.float32 and bool((xy >= ref.XY_LO).all()) and bool((xy <= ref.XY_HI).all())
    if fixed is None:
        fidx = fidx.cpu()
        assert fidx.dtype == torch.long and bool(((fidx >= 0) & (fidx < V)).all())
        Ci = torch.cat([torch.zeros(1, dtype=torch.float64), ref.cdf_image(em0)])
        e = V * U
        assert bool(((Ci[fidx] - e <= u[:, 0]) & (u[:, 0] <= Ci[fidx + 1] + e)).all())
    else:
        fidx = torch.full([xy.shape[0]], fixed, dtype=torch.long)
    _, cx, cy = ref.cells(fidx, xy, h, w)              # int(x w), int(y h): the cell the update will account this pixel to
    c = cy * w + cx
    Cc = torch.cat([torch.zeros([V, 1], dtype=torch.float64), ref.cdf_cell(em0, min_pdf, max_pdf)], dim=1)
    e = h * w * U
    ok = (Cc[fidx, c] - e <= u[:, 1]) & (u[:, 1] <= Cc[fidx, c + 1] + e)
    assert bool(ok.all()), int((~ok).sum())
    return fidx, c


@pytest.mark.parametrize("hw", [(3, 5), (32, 64), (48, 64)])
def test_draw_rows_follow_the_cdfs(backend, hw):
    V, n = 5, 2048
    em, _ = _maps(V, hw, backend, seed=11, kind="zeros", min_pdf=0.01)
    smp = ImpSampler({"error_map": (em, 1.0)}, frac_uniform=0.0)
    g = torch.Generator().manual_seed(12)
    u = torch.stack([_stratified(n, g), _stratified(n, g), torch.rand([n], generator=g), torch.rand([n], generator=g)], dim=-1)
    fidx, xy = smp.sample_img_pixel(n, u.to(backend))
    sync(backend)
    _check_rows(fidx, xy, u, em.error_map, hw, 0.01)
    # edge rows: every combination of the extreme uniforms
    ev = torch.tensor([0.0, U, 1.0 - U])
    ue = torch.cartesian_prod(ev, ev, torch.tensor([0.0, 1.0 - U]), torch.tensor([0.0, 0.5, 1.0 - U])).contiguous()
    fe, xe = smp.sample_img_pixel(ue.shape[0], ue.to(backend))
    sync(backend)
    f_, c_ = _check_rows(fe, xe, ue, em.error_map, hw, 0.01)
    assert int(c_.min()) >= 0 and int(c_.max()) < hw[0] * hw[1]
    # the position inside the cell is the jitter: x w - cx = u2 up to the rounding of x
    # (rounding of cx + u2 to f32, of the quotient, and at most a few ulps of nudging: 4 u w; rows on the clamp excepted)
    _, cx, cy = ref.cells(fidx, xy, *hw)
    x, y = xy.cpu()[:, 0].double(), xy.cpu()[:, 1].double()
    free = (xy.cpu() > ref.XY_LO).all(-1) & (xy.cpu() < ref.XY_HI).all(-1)
    assert int(free.sum()) > n - 8
    assert float(((x * hw[1] - cx) - u[:, 2].double()).abs()[free].max()) <= 4 * U * hw[1]
    assert float(((y * hw[0] - cy) - u[:, 3].double()).abs()[free].max()) <= 4 * U * hw[0]


def test_draw_fixed_frame_counts(backend):
    V, hw, n, fi = 5, (32, 64), 4096, 3
    em, em0 = _maps(V, hw, backend, seed=13, kind="zeros", min_pdf=0.01)
    smp = ImpSampler({"error_map": (em, 1.0)}, frac_uniform=0.0)
    g = torch.Generator().manual_seed(14)
    u = torch.stack([torch.rand([n], generator=g), _stratified(n, g), torch.rand([n], generator=g), torch.rand([n], generator=g)], -1)
    xy = smp.sample_pixel(n, fi, u.to(backend))
    sync(backend)
    assert xy.shape == (n, 2) and xy.dtype == torch.float32
    _, c = _check_rows(None, xy, u, em.error_map, hw, 0.01, fixed=fi)
    count = torch.bincount(c, minlength=hw[0] * hw[1]).double()
    p = ref.pdf(em0, 0.01)[fi].reshape(-1)
    eps = hw[0] * hw[1] * U
    assert bool(((count - n * p).abs() <= 1 + 2 * n * eps).all()), float((count - n * p).abs().max())


def test_draw_uniform_share_and_split(backend):
    from nr3d_lib.models.importance import TorchErrorMap, TorchImpSampler
    V, hw, n = 5, (32, 64), 1001
    em, _ = _maps(V, hw, backend, seed=15, min_pdf=0.01)
    smp = ImpSampler({"error_map": (em, 1.0)}, frac_uniform=0.25)
    tsm = TorchImpSampler({"error_map": (TorchErrorMap(V, error_map_hw=hw), 1.0)}, frac_uniform=0.25)
    for k in (0, 1, 2, 7, 1001, 4096, 8191):
        assert smp._split(k) == tsm._split(k)
    n_uni, parts = smp._split(n)
    assert n_uni == round(n * 0.25) == 250 and parts == {"error_map": 751}
    g = torch.Generator().manual_seed(16)
    u = torch.rand([n, 4], generator=g)
    fidx, xy = smp.sample_img_pixel(n, u.to(backend))
    sync(backend)
    f_ref, xy_ref = ref.uniform_rows(u[:n_uni], V)
    assert torch.equal(fidx.cpu()[:n_uni], f_ref) and torch.equal(xy.cpu()[:n_uni], xy_ref)
    _check_rows(fidx[n_uni:], xy[n_uni:], u[n_uni:], em.error_map, hw, 0.01)
    # fixed frame: the uniform rows keep the frame, xy by the same formula
    xy1 = smp.sample_pixel(n, 2, u.to(backend))
    sync(backend)
    assert torch.equal(xy1.cpu()[:n_uni], xy_ref)
    _check_rows(None, xy1[n_uni:], u[n_uni:], em.error_map, hw, 0.01, fixed=2)
    # u = None: one draw on the device, same shapes and ranges
    f2, xy2 = smp.sample_img_pixel(n)
    assert f2.shape == (n,) and f2.dtype == torch.long and xy2.shape == (n, 2) and xy2.dtype == torch.float32
    assert f2.device.type == backend.type and bool(((xy2 > 0) & (xy2 < 1)).all()) and bool(((f2 >= 0) & (f2 < V)).all())


def test_draw_two_maps_fill_disjoint_row_ranges(backend):
    from nr3d_lib.models.importance import TorchErrorMap, TorchImpSampler
    V, hw, n = 5, (4, 8), 1000
    a, b = ErrorMap(V, error_map_hw=hw, device=backend), ErrorMap(V, error_map_hw=hw, device=backend)
    with torch.no_grad():            # all of map a's mass in image 0, all of map b's in image 4
        a.error_map.zero_()
        a.error_map[0] = 1.0
        b.error_map.zero_()
        b.error_map[4, 1, 2] = 1.0
    a.invalidate()
    b.invalidate()
    smp = ImpSampler({"a": (a, 0.3), "b": (b, 0.2)}, frac_uniform=0.5)
    tsm = TorchImpSampler({"a": (TorchErrorMap(V, error_map_hw=hw), 0.3), "b": (TorchErrorMap(V, error_map_hw=hw), 0.2)}, 0.5)
    n_uni, parts = smp._split(n)
    assert (n_uni, parts) == tsm._split(n) == (500, {"a": 300, "b": 200})
    u = torch.rand([n, 4], generator=torch.Generator().manual_seed(17))
    fidx, xy = smp.sample_img_pixel(n, u.to(backend))
    sync(backend)
    fidx = fidx.cpu()
    assert torch.equal(fidx[:500], ref.uniform_rows(u[:500], V)[0])
    assert bool((fidx[500:800] == 0).all()) and bool((fidx[800:] == 4).all())
    _check_rows(fidx[500:800], xy[500:800], u[500:800], a.error_map, hw, 0.01)
    _, c = _check_rows(fidx[800:], xy[800:], u[800:], b.error_map, hw, 0.01)
    assert float((c == 1 * 8 + 2).float().mean()) > 0.9                     # (the other cells hold min_pdf / (h w) each)
    pi = smp.get_pdf_image().cpu()
    assert torch.allclose(pi, torch.tensor([0.3, 0, 0, 0, 0.2]), atol=1e-6)


def test_product_refuses_cpu_tensors():
    """No CPU fallback (the product loader, no backend fixture): every public op raises on host tensors."""
    em = ErrorMap(2, error_map_hw=(4, 4))
    smp = ImpSampler({"error_map": (em, 1.0)})
    xy, v = torch.rand([8, 2]), torch.rand([8])
    for f in (lambda: em.step_error_map(torch.zeros([8], dtype=torch.long), xy, v),
              lambda: em.step_error_map_rgb(torch.zeros([8], dtype=torch.long), xy, torch.rand([8, 3]), torch.rand([8, 3]), "mse"),
              lambda: em.get_pdf(), lambda: em.get_pdf_image(), lambda: smp.sample_img_pixel(8, torch.rand([8, 4])),
              lambda: smp.sample_pixel(8, 0, torch.rand([8, 4])), lambda: smp.sample_img_pixel(8)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


# ----------------------------------------------------------------------------------------------------------- trainer
def _trainer(backend, seed=42, **kw):
    from neuralsim_amd.graphics.cameras import look_at_cameras
    from neuralsim_amd.trainer import RenderTrainer
    from test_trainer import _tiny
    torch.manual_seed(0)                    # the occupancy initialisation draws from the global generator
    m = _tiny(backend, seed=seed)
    intr, c2w, WH = look_at_cameras(V=4, seed=1, device=backend)
    args = dict(num_rays=40, lr=2e-3, num_uniform=24, perturb=True, target_sphere_radius=0.5)
    args.update(kw)
    return RenderTrainer(m, intr, c2w, WH, **args)


def test_trainer_before_enable_after_draws_the_uniform_batch(backend):
    tr_e = _trainer(backend, pixel_sample_mode="error_map", error_map=dict(error_map_hw=(8, 8), enable_after=10 ** 9))
    tr_u = _trainer(backend)
    assert tr_u.imp_sampler is None and tr_u.error_map is None and tr_e.error_map.error_map.shape == (4, 8, 8)
    for _ in range(2):
        be, bu = tr_e._make_batch(), tr_u._make_batch()
        for k in ("xy", "fidx", "gt"):
            assert torch.equal(be[k], bu[k]), k
    with pytest.raises(ValueError):
        _trainer(backend, pixel_sample_mode="errormap")


def test_trainer_one_step_updates_the_map_on_both_paths(backend, monkeypatch):
    from neuralsim_amd.trainer import RenderTrainer
    seen = {}
    real_loss = RenderTrainer.loss

    def spy(self, ret, gt, *a, **k):
        seen["rgb"], seen["gt"] = ret["rendered"]["rgb_volume"].detach().clone(), gt.detach().clone()
        return real_loss(self, ret, gt, *a, **k)
    monkeypatch.setattr(RenderTrainer, "loss", spy)
    outs = {}
    for fused in (True, False):
        tr = _trainer(backend, fused_step=fused, pixel_sample_mode="error_map",
                      error_map=dict(error_map_hw=(8, 8), enable_after=0, frac_uniform=0.5))
        assert tr._fused_ok() == fused
        loss = float(tr.train_step(0))
        sync(backend)
        fidx, xy, err = tr.last_batch_error
        assert loss == loss and err.shape == (40,) and not err.requires_grad
        r, ns, c = ref.update(torch.ones([4, 8, 8], dtype=torch.float64), torch.zeros([4], dtype=torch.long), fidx, xy, err)
        _check_update(tr.error_map.error_map, r, c, torch.ones([4, 8, 8]), max(1.0, float(err.max())))
        assert torch.equal(tr.error_map.n_steps.cpu(), ns)
        outs[fused] = (fidx.cpu(), xy.cpu(), err.cpu())
    assert "rgb" in seen                                                 # (the autograd path went through ``loss``)
    e64 = ref.rgb_error(seen["rgb"], seen["gt"], "mse")
    assert bool(((outs[False][2].double() - e64).abs() <= 7 * U * e64).all())
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])      # same seed, same batch
    ea, eb = outs[True][2], outs[False][2]
    assert float(eb.max()) > 0 and bool(((ea - eb).abs() <= 1e-5 * (1 + eb.abs())).all()), float((ea - eb).abs().max())


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_train_steps_with_error_map_sampling(backend, fused):
    hw, V, N = (2, 2), 4, 48
    tr = _trainer(backend, fused_step=fused, pipeline=True, num_rays=N, pixel_sample_mode="error_map",
                  error_map=dict(error_map_hw=hw, enable_after=0, frac_uniform=0.5, min_pdf=0.0))
    n_uni = tr.imp_sampler._split(N)[0]
    touched = torch.zeros([V * hw[0] * hw[1]], dtype=torch.bool)
    complete_at = None
    for it in range(8):
        loss = float(tr.train_step(it))
        sync(backend)
        fidx, xy, err = (t.cpu() for t in tr.last_batch_error)
        assert loss == loss and bool(torch.isfinite(xy).all()) and bool(((xy > 0) & (xy < 1)).all())
        assert fidx.dtype == torch.long and bool(((fidx >= 0) & (fidx < V)).all()) and bool(torch.isfinite(err).all())
        em = tr.error_map.error_map.cpu()
        assert bool(torch.isfinite(em).all()) and bool((em >= 0).all())
        flat, _, _ = ref.cells(fidx, xy, *hw)
        if bool(touched.all()):          # every cell has been hit: no non-uniform row can fall into a never-touched cell
            complete_at = it if complete_at is None else complete_at
            assert float((~touched[flat[n_uni:]]).float().mean()) == 0.0
        touched[flat] = True
    assert complete_at is not None and complete_at <= 4, complete_at
    assert int(tr.error_map.n_steps.sum()) > 8 and tr._fused_ok() == fused


def test_shim_reexports_the_hip_classes_on_request(monkeypatch):
    import nr3d_lib.models.importance as shim
    try:
        monkeypatch.delenv("NSIM_IMP_SAMPLER", raising=False)
        shim = importlib.reload(shim)
        assert shim.ImpSampler is shim.TorchImpSampler and shim.ErrorMap is shim.TorchErrorMap
        assert shim.ImpSampler is not ImpSampler and shim.ImpSampler.__module__ == "nr3d_lib.models.importance"
        monkeypatch.setenv("NSIM_IMP_SAMPLER", "hip")
        shim = importlib.reload(shim)
        assert shim.ImpSampler is ImpSampler and shim.ErrorMap is ErrorMap
        assert shim.TorchImpSampler.__module__ == "nr3d_lib.models.importance"
    finally:
        monkeypatch.undo()
        importlib.reload(shim)
