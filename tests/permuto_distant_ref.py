"""CPU specification of ``PermutoNeRFDistantModel`` and of hardmask level annealing on the permutohedral lattice, composed
from the existing oracles (TEST INFRASTRUCTURE):

* encoding: ``oracle.permuto.permuto_forward`` on x = 2 u4 - 1 (u4 in [0,1]^4 as ``oracle.distant.shell_points_u4`` gives
  it), with a level mask that zeroes the features of levels >= n_active -- a masked level then has no gradient at all;
* everything else: ``oracle.distant``'s shells, decoders and ``density_alpha``, unchanged (``distant_ray_query`` with the
  encoding swapped).

The nr3d_lib implementation is absent: the input convention is fixed by this project.
"""
import contextlib
from unittest import mock

import torch

from oracle import distant as od, permuto as operm

_permuto_forward = operm.permuto_forward


def masked_permuto_forward(x, params, spec, n_active=None):
    """``permuto_forward`` with hardmask annealing: features of levels >= n_active are zero (None / >= L: all levels)."""
    out = _permuto_forward(x, params, spec)
    if n_active is None or n_active >= spec.num_levels:
        return out
    keep = torch.zeros(spec.out_features, dtype=out.dtype)
    keep[:spec.n_feats * max(1, int(n_active))] = 1.0
    return out * keep


@contextlib.contextmanager
def masked_levels(n_active):
    """Inside: every oracle that encodes through ``oracle.permuto.permuto_forward`` (``oracle.field.encode``) sees the mask."""
    with mock.patch.object(operm, "permuto_forward",
                           lambda x, params, spec: masked_permuto_forward(x, params, spec, n_active)):
        yield


def make_permuto_distant_params(cfg: dict, seed=7, grid_bound=0.5, use_view_dirs=True) -> od.DistantParams:
    """``oracle.distant.DistantParams`` whose ``spec`` is a 4-D ``PermutoSpec`` (``cfg``: permuto_auto_compute_cfg)."""
    spec = operm.make_permuto_spec(in_dim=4, **{k: v for k, v in cfg.items() if k != "type"})
    # ``make_distant_params`` reads num_levels / n_params of the spec only
    return od.make_distant_params(spec, seed=seed, grid_bound=grid_bound, use_view_dirs=use_view_dirs)


def distant_ray_query(p: od.DistantParams, *args, n_active=None, **kw):
    """``oracle.distant.distant_ray_query`` with the 4-D LoTD gather replaced by the (masked) lattice on 2 u4 - 1.  The
    lattice runs on f64 inputs so that 2 u - 1 is exact, as the kernel's folded scale / shift computes it."""
    def enc(u4, grid, spec):
        return masked_permuto_forward(2.0 * u4.double() - 1.0, grid.double(), spec, n_active).float()
    with mock.patch.object(od, "lotd4_forward", enc):
        return od.distant_ray_query(p, *args, **kw)
