"""Reference for the table gathers (tests/test_table_gather.py): per kernel family the float64 features, d features / d x
and (3-D LoTD) the mixed-second-derivative planes of every (level, sample, feature), with the ingredients of the error bound
that goes with them.  Inputs are what the kernel is given: the f32 points (``scatter_ref.SampleSet.points(form)``) and the
fp16 table, widened.  The cell rule is the kernels' (lotd_dev.h / nerf_field.hip ``lotd4_cell``):

    pos = u (R - 1),  c0 = clamp(floor(pos), 0, R - 2),  w = pos - c0      (w = 1 on the top face, outside [0, 1] beyond the box)

The vertex and weight arithmetic restates oracle/lotd.py, oracle/distant.py::lotd4_forward and oracle/permuto.py (whose own
``_vertex_index`` / ``simplex`` / ``barycentric`` / ``vertex_index`` are called);
tests/test_table_gather.py::test_reference_equals_oracle ties every array to those oracles and to autograd through them.

Bound per (level, sample, feature), derived, not measured:

    |got - ref| <= (r_l + 16) 2^-24 W A

A = sum of |table value| over the vertices of the sample's cell (simplex); W = prod_a (|w_a| + |1 - w_a|): 1 inside the cell,
growing where the interpolant extrapolates beyond the box (the sum of the |weights|); r_l: the error of the weights, which is
the absolute error of ``pos`` -- three roundings at a size up to R_l on each of three axes: 9 R_l; 12 R_l for the 4-D
pyramid; (in_dim + 1) x the level's largest scale on the permutohedral lattice (scatter_ref's ``rterm``; its elevation runs
in f64, what remains is the input's rounding) -- and 16 for the eight- / sixteen-term f32 sums and products themselves.
d features / d x_a: the same times dscale_a = x_scale_a (R_a - 1) (the lattice: scale_a).  The hess contraction: the same
times the two dscale factors, |g| and |gn|, summed over the levels in f32 (+ L in the constant) into a pre-filled dx (one more
rounding at the size of the result).  An f16 output adds the conversion's half ulp: 2^-11 relative (2^-25 absolute in the
subnormal range) at the size of the converted value.
"""
from dataclasses import dataclass
from typing import Optional

import torch

import scatter_ref as sr
from scatter_ref import EPS, F64
from oracle import distant as odist, lotd as olotd, permuto as operm

F16_REL = 2.0 ** -11          # half an ulp of a normal f16, relative
F16_SUB = 2.0 ** -25          # half the spacing of the f16 subnormals
F16_MAX = 65504.0             # field.hip f16_sat
H_SCALE = 1024.0              # field.hip SDF_H_SCALE = permuto.hip PERMUTO_SDF_H_SCALE


@dataclass
class GatherRef:
    feat: torch.Tensor                    # [L, S, 2] f64
    J: Optional[torch.Tensor]             # [L, S, 2, 3] f64: d feat / d x (None: 4-D)
    H: Optional[torch.Tensor]             # [L, S, 2, 3] f64: d2 feat / dx dy, dx dz, dy dz (3-D LoTD only)
    A: torch.Tensor                       # [L, S, 2]
    W: torch.Tensor                       # [L, S]
    rl: torch.Tensor                      # [L]
    dsc: Optional[torch.Tensor]           # [L, 3]

    def feat_bound(self):
        return ((self.rl + 16.0) * EPS)[:, None, None] * self.W[:, :, None] * self.A

    def J_bound(self):
        return self.feat_bound()[..., None] * self.dsc[:, None, None, :]


def f16_term(ref, bnd, scale=1.0):
    """what the conversion f16(sat(scale * v)) adds to the bound of v (in units of v): half an f16 ulp at the size of the
    converted value -- the reference's plus the bound it may be off by"""
    return torch.maximum(F16_REL * (ref.abs() + bnd), torch.full_like(ref, F16_SUB / scale))


def f16_sat(ref, scale=1.0):
    """the value an f16 plane holds for v: clamp(scale v, +-65504) / scale (the clamp is 1-Lipschitz: the bound carries over)"""
    return (ref * scale).clamp(-F16_MAX, F16_MAX) / scale


# ===================================================================================================== 3-D LoTD
def lotd_ref(lv: sr.LotdLevels, table, p, goff=None, n_active=None) -> GatherRef:
    """table: flat fp16 (all instances); p [S, 3] f64; goff [S] int64 (scalars) or None; levels >= n_active: zeros"""
    tab = table.double()
    S, L = p.shape[0], lv.num_levels
    goff = torch.zeros(S, dtype=torch.long) if goff is None else goff
    feat, J, H, A = (torch.zeros(L, S, 2, dtype=F64), torch.zeros(L, S, 2, 3, dtype=F64), torch.zeros(L, S, 2, 3, dtype=F64),
                     torch.zeros(L, S, 2, dtype=F64))
    W = torch.ones(L, S, dtype=F64)
    rl = torch.tensor([9.0 * max(r) for r in lv.res3], dtype=F64)
    dsc = torch.stack([torch.tensor(lv.xs, dtype=F64) * (torch.tensor(r, dtype=F64) - 1.0) for r in lv.res3])
    for l in range(L if n_active is None else min(n_active, L)):
        pos, R3 = sr._lotd_pos(lv, p, l)
        c0 = torch.minimum(torch.floor(pos).clamp_min(0), R3 - 2.0)
        w = pos - c0
        c0 = c0.long()
        W[l] = (w.abs() + (1.0 - w).abs()).prod(-1)
        for corner in range(8):
            b = [(corner >> a) & 1 for a in range(3)]
            wa = [w[:, a] if b[a] else 1.0 - w[:, a] for a in range(3)]
            sg = [1.0 if b[a] else -1.0 for a in range(3)]
            idx = olotd._vertex_index(c0[:, 0] + b[0], c0[:, 1] + b[1], c0[:, 2] + b[2], lv.res3[l], lv.types[l], lv.hashmap_size)
            base = goff + lv.offsets[l] + 2 * idx
            v = torch.stack([tab[base], tab[base + 1]], dim=-1)                          # [S, 2]
            feat[l] += (wa[0] * wa[1] * wa[2])[:, None] * v
            A[l] += v.abs()
            dw = [sg[0] * wa[1] * wa[2], sg[1] * wa[0] * wa[2], sg[2] * wa[0] * wa[1]]
            for a in range(3):
                J[l, :, :, a] += (dw[a] * dsc[l, a])[:, None] * v
            for k, (a, b2, c) in enumerate(((0, 1, 2), (0, 2, 1), (1, 2, 0))):            # pair (a, b2), third axis c
                H[l, :, :, k] += (sg[a] * sg[b2] * wa[c] * dsc[l, a] * dsc[l, b2])[:, None] * v
    return GatherRef(feat, J, H, A, W, rl, dsc)


def hess_dx(ref: GatherRef, g, gn, dx0):
    """nsim_lotd_hess_dx: dx0[s][c] + sum_{l,f} g[l,s,f] sum_{c' != c} gn[s,c'] d2 h_{l,f} / dx_c' dx_c -> (value, bound) [S, 3].
    g [L, S, 2], gn, dx0 [S, 3], all f64."""
    h = (g[..., None] * ref.H).sum(2)                                                     # [L, S, 3]: xy, xz, yz
    hxy, hxz, hyz = h[..., 0].sum(0), h[..., 1].sum(0), h[..., 2].sum(0)
    acc = torch.stack([gn[:, 1] * hxy + gn[:, 2] * hxz, gn[:, 0] * hxy + gn[:, 2] * hyz, gn[:, 0] * hxz + gn[:, 1] * hyz], dim=-1)
    L = ref.feat.shape[0]
    B = ((ref.rl + 16.0 + L) * EPS)[:, None] * ref.W * (g.abs() * ref.A).sum(-1)          # [L, S]
    d = ref.dsc
    pxy, pxz, pyz = ((B * (d[:, i] * d[:, j])[:, None]).sum(0) for i, j in ((0, 1), (0, 2), (1, 2)))
    a = gn.abs()
    bnd = torch.stack([a[:, 1] * pxy + a[:, 2] * pxz, a[:, 0] * pxy + a[:, 2] * pyz, a[:, 0] * pxz + a[:, 1] * pyz], dim=-1)
    val = dx0 + acc
    return val, bnd + EPS * (dx0.abs() + acc.abs())


# ===================================================================================================== 4-D LoTD
def lotd4_ref(spec: odist.LoTD4Spec, table, u) -> GatherRef:
    """u [S, 4] f64 (any value: the cell is clamped, the interpolant extrapolates)"""
    tab = table.double()
    S, L = u.shape[0], spec.num_levels
    feat, A = torch.zeros(L, S, 2, dtype=F64), torch.zeros(L, S, 2, dtype=F64)
    W = torch.ones(L, S, dtype=F64)
    rl = torch.tensor([12.0 * max(spec.res_of(l)) for l in range(L)], dtype=F64)
    m = 0xFFFFFFFF
    for l in range(L):
        R4 = spec.res_of(l)
        R = torch.tensor(R4, dtype=F64)
        pos = u * (R - 1.0)
        c0 = torch.minimum(torch.floor(pos).clamp_min(0), R - 2.0)
        w = pos - c0
        c0 = c0.long()
        W[l] = (w.abs() + (1.0 - w).abs()).prod(-1)
        for corner in range(16):
            b = [(corner >> a) & 1 for a in range(4)]
            wt = torch.ones(S, dtype=F64)
            for a in range(4):
                wt = wt * (w[:, a] if b[a] else 1.0 - w[:, a])
            c = [c0[:, a] + b[a] for a in range(4)]
            if spec.types[l] == "Dense":
                idx = c[0] + R4[0] * (c[1] + R4[1] * (c[2] + R4[2] * c[3]))
            else:
                P = odist.PRIMES4
                idx = (((c[0] * P[0]) & m) ^ ((c[1] * P[1]) & m) ^ ((c[2] * P[2]) & m) ^ ((c[3] * P[3]) & m)) % spec.hashmap_size
            base = spec.offsets[l] + 2 * idx
            v = torch.stack([tab[base], tab[base + 1]], dim=-1)
            feat[l] += wt[:, None] * v
            A[l] += v.abs()
    return GatherRef(feat, None, None, A, W, rl, None)


# ===================================================================================================== permutohedral lattice
def permuto_ref(pm: sr.PermutoLevels, table, p, n_active=None) -> GatherRef:
    """p [S, in_dim] f64 (the condition appended); J: d feat / d x[:3]"""
    S, L, n = p.shape[0], pm.num_levels, pm.in_dim + 1
    tab = table.double().view(L, pm.T, 2)
    feat, J, A = torch.zeros(L, S, 2, dtype=F64), torch.zeros(L, S, 2, 3, dtype=F64), torch.zeros(L, S, 2, dtype=F64)
    rl = torch.tensor([n * float(pm.scale[l].max()) for l in range(L)], dtype=F64)
    for l in range(L if n_active is None else min(n_active, L)):
        rem0, rank, bary, dB = sr._permuto_level(pm, p, l)
        for r in range(n):
            v = tab[l][operm.vertex_index(rem0, rank, r, pm.T)]
            feat[l] += bary[:, r, None] * v
            A[l] += v.abs()
            J[l] += v[:, :, None] * dB[:, r, None, :3]
    return GatherRef(feat, J, None, A, torch.ones(L, S, dtype=F64), rl, pm.scale[:, :3].clone())


# ===================================================================================================== the sets
def whole_box(n, dim=3, box=(-1.0, 1.0), seed=31) -> sr.SampleSet:
    """n points over the whole box and beyond: every corner, the face / edge centres and dyadic interior points first (3^dim
    then 2 * 3^dim lattice points, cut to n), the rest uniform over +-1.2 half widths -- outside the box the interpolant
    extrapolates.  One ray per point through it (t != 0: the ray form rounds; t = 0 on the special points, which both forms then
    hit exactly)."""
    lo, hi = sr._box(dim, box)
    mid, half = (lo + hi) * 0.5, (hi - lo) * 0.5
    ax = torch.tensor([-1.0, 0.0, 1.0], dtype=F64)
    faces = torch.cartesian_prod(*([ax] * dim)).reshape(-1, dim)
    dy = torch.cartesian_prod(*([torch.tensor([-0.5, 0.25, 0.75], dtype=F64)] * dim)).reshape(-1, dim)
    g = torch.Generator().manual_seed(seed)
    special = torch.cat([faces, dy, faces[torch.randperm(faces.shape[0], generator=g)] * 1.125])
    k = min(n // 2, special.shape[0])
    unit = torch.cat([special[torch.randperm(special.shape[0], generator=g)[:k]],
                      (torch.rand(n - k, dim, generator=g, dtype=F64) * 2 - 1) * 1.2])
    unit = unit[torch.randperm(n, generator=g)]
    pts = (mid + unit * half).float()
    d = sr._unit(sr._DIR[:dim]).float().expand(n, dim).contiguous()
    t = (0.25 * float(half.min()) * torch.rand(n, generator=g)).float()
    t[(unit.abs() <= 1.125).all(-1) & (unit * 8 == (unit * 8).round()).all(-1)] = 0.0      # the special points: exact in both forms
    o = (pts.double() - t.double()[:, None] * d.double()).float()
    return sr.SampleSet(f"box{n}", o, d, t, torch.arange(n), torch.ones(n, dtype=torch.bool))


def ratio(err, bnd):
    """worst error / bound (0 / 0: exact; a NaN anywhere: inf)"""
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    return float(r.max())
