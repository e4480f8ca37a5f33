"""Error-map importance sampling of training pixels on the HIP kernels of csrc/sampling.hip (``nsim_errmap_*``).

``ErrorMap`` / ``ImpSampler`` keep the constructor signatures, buffers and methods of ``nr3d_lib.models.importance`` (the reference's
trainer builds one sampler per camera, code_single/tools/train.py:105-138; the joint-frame pixel loader draws (frame, pixel) from it
once per iteration, dataio/data_loader/pixel_loader.py:157-171, 280-302; the trainer scatters the batch's per-ray photometric error
back, train.py:619-621, 678-688).  What differs from the torch classes:

* a draw is TWO-LEVEL -- the image by its share of the map's mass, then the cell by the image's pdf: the joint pdf
  ``pdf[i, c] * pdf_image[i]`` the torch classes hand to ``torch.multinomial`` -- from explicit uniforms ``u`` [n, 4] (image, cell,
  jitter x, jitter y; ``None``: one ``torch.rand`` on the device), two binary searches per ray instead of a multinomial over all
  ``n_images h w`` cells;
* an update is two launches (f32 atomics into scratch planes that stay zero between calls, then the blend), and
  ``step_error_map_rgb`` takes the rendered and the target colours and computes the per-ray error in the same launch;
* the CDF tables are rebuilt lazily -- by the first reader after an update -- into one of TWO alternating snapshots, so a reader on
  another stream keeps a table nobody writes (see ``cdfs``).
"""
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib

_FN = {"mse": 0, "l1": 1}


def _f32(t: torch.Tensor, cols: int, name: str) -> torch.Tensor:
    """t as a detached, contiguous float32 [N, cols] ([N] for cols 0) device tensor -- itself when it already is one (the trainer's
    per-step call: no tensor op at all)"""
    _lib.require_device(t, name)
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if (t.dim() != 1) if cols == 0 else (t.dim() != 2 or t.shape[1] != cols):
        t = t.reshape(-1) if cols == 0 else t.reshape(-1, cols)
    return t if t.is_contiguous() else t.contiguous()


class ErrorMap(nn.Module):
    def __init__(self, n_images: int, error_map_hw=(32, 32), n_steps_max: int = None, n_steps_init: int = 0,
                 min_pdf: float = 0.01, max_pdf: float = None, dtype=torch.float32, device=None, **unused):
        super().__init__()
        if dtype != torch.float32:
            raise TypeError(f"neuralsim_amd: the error map is float32 (got {dtype})")
        self.n_images, (self.h, self.w) = int(n_images), (int(error_map_hw[0]), int(error_map_hw[1]))
        if self.n_images < 1 or self.h < 1 or self.w < 1 or self.n_images * self.h * self.w >= 2 ** 31:
            raise ValueError("neuralsim_amd: error map needs n_images, h, w >= 1 and n_images * h * w < 2^31")
        self.n_steps_max = n_steps_max
        self.min_pdf, self.max_pdf = float(min_pdf), (float(max_pdf) if max_pdf is not None else None)
        n_cells = self.n_images * self.h * self.w
        self.register_buffer("error_map", torch.ones([self.n_images, self.h, self.w], dtype=dtype, device=device))
        self.register_buffer("n_steps", torch.full([self.n_images], int(n_steps_init), dtype=torch.long, device=device))
        # scratch of the update: zero between calls (nsim_errmap_blend re-zeroes what it consumed)
        self.register_buffer("_sum", torch.zeros([n_cells], dtype=torch.float32, device=device), persistent=False)
        self.register_buffer("_cnt", torch.zeros([n_cells], dtype=torch.float32, device=device), persistent=False)
        self.register_buffer("_touched", torch.zeros([self.n_images], dtype=torch.int32, device=device), persistent=False)
        self._snaps, self._cur, self._dirty = [None, None], 0, True

    # ---------------------------------------------------------------------------------------------- update
    def _frames(self, i, n: int):
        if isinstance(i, torch.Tensor):
            _lib.require_device(i, "i")
            if i.dtype == torch.long and i.dim() == 1 and i.shape[0] == n and n > 1 and i.is_contiguous():
                return i, 1
        i = torch.as_tensor(i, device=self.error_map.device).reshape(-1).long()
        if i.numel() != n and i.numel() != 1:
            raise ValueError(f"neuralsim_amd: {i.numel()} frame indices for {n} pixels")
        return i.contiguous(), (1 if i.numel() == n and n > 1 else 0)

    def _step(self, i, xy, val, pred, gt, fn, want_err):
        xy = _f32(xy, 2, "xy")
        n = int(xy.shape[0])
        _lib.require_device(self.error_map, "error_map")
        i, stride = self._frames(i, n)
        err = torch.empty([n], dtype=torch.float32, device=xy.device) if want_err else None
        if n == 0:
            return err
        _lib.call("nsim_errmap_accumulate", i, stride, xy, val, pred, gt, int(fn), n, self.n_images, self.h, self.w,
                  self._sum, self._cnt, self._touched, err)
        _lib.call("nsim_errmap_blend", self.error_map, self._sum, self._cnt, self._touched, self.n_steps, self.n_images,
                  self.h, self.w)
        self._dirty = True
        return err

    @torch.no_grad()
    def step_error_map(self, i: torch.Tensor, xy: torch.Tensor, val: torch.Tensor):
        """i: frame [N] (or one frame for all), xy [N,2] in [0,1], val [N]: mean per cell, blended half and half into the map."""
        self._step(i, xy, _f32(val, 0, "val"), None, None, 0, False)

    @torch.no_grad()
    def step_error_map_rgb(self, i: torch.Tensor, xy: torch.Tensor, pred: torch.Tensor, gt: torch.Tensor, fn: str = "mse"):
        """``step_error_map`` with val = mean_c fn(pred - gt) of pred / gt [N,3] (fn ``mse`` | ``l1``) computed by the update's own
        launch; -> that per-ray error [N]."""
        if fn not in _FN:
            raise ValueError(f"neuralsim_amd: rgb error function must be one of {sorted(_FN)}, got {fn!r}")
        return self._step(i, xy, None, _f32(pred, 3, "pred"), _f32(gt, 3, "gt"), _FN[fn], True)

    def invalidate(self):
        """Call after writing ``error_map`` directly (``load_state_dict`` does): the next reader rebuilds the tables."""
        self._dirty = True

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._dirty = True

    # ---------------------------------------------------------------------------------------------- tables
    def _new_snap(self):
        dev, V, hw = self.error_map.device, self.n_images, self.h * self.w
        f32 = dict(dtype=torch.float32, device=dev)
        return dict(cdf_cell=torch.empty([V, hw], **f32), pdf_cell=torch.empty([V, hw], **f32), mass=torch.empty([V], **f32),
                    cdf_img=torch.empty([V], **f32), pdf_img=torch.empty([V], **f32))

    @torch.no_grad()
    def tables(self) -> dict:
        """The current snapshot {cdf_cell [V, h w], pdf_cell, mass [V], cdf_img [V], pdf_img [V]}.  When the map changed since the
        last call the tables are rebuilt -- on the caller's stream -- into the OTHER of two snapshots, which then becomes current:
        whoever still reads the previous snapshot (a draw queued on another stream) is not disturbed, provided it is done before
        the rebuild after the next one starts.  ``RenderTrainer`` states how its streams guarantee that."""
        _lib.require_device(self.error_map, "error_map")
        if self._dirty or self._snaps[self._cur] is None or self._snaps[self._cur]["mass"].device != self.error_map.device:
            nxt = 1 - self._cur
            if self._snaps[nxt] is None or self._snaps[nxt]["mass"].device != self.error_map.device:
                self._snaps[nxt] = self._new_snap()
            s = self._snaps[nxt]
            _lib.call("nsim_errmap_cdf", self.error_map, self.n_images, self.h, self.w, self.min_pdf,
                      -1.0 if self.max_pdf is None else self.max_pdf, s["cdf_cell"], s["pdf_cell"], s["mass"], s["cdf_img"],
                      s["pdf_img"])
            self._cur, self._dirty = nxt, False
        return self._snaps[self._cur]

    def cdfs(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (cdf_img [n_images], cdf_cell [n_images, h w]) of the current snapshot (see ``tables``)."""
        t = self.tables()
        return t["cdf_img"], t["cdf_cell"]

    def get_pdf(self, fi=None) -> torch.Tensor:
        """-> [n, h, w] (fi given) or [n_images, h, w] probabilities, each image's cells summing to 1."""
        p = self.tables()["pdf_cell"].view(self.n_images, self.h, self.w)
        return p.clone() if fi is None else p[torch.as_tensor(fi, device=p.device).reshape(-1)]

    def get_normalized_error_map(self, fi) -> torch.Tensor:
        em = self.error_map[int(fi)]
        return em / em.max().clamp_min(1e-12)

    def get_pdf_image(self) -> torch.Tensor:
        return self.tables()["pdf_img"].clone()


class ImpSampler(nn.Module):
    def __init__(self, error_maps: Dict[str, Tuple[ErrorMap, float]], frac_uniform: float = 0.5):
        super().__init__()
        self.error_maps = nn.ModuleDict({k: v[0] for k, v in error_maps.items()})
        self.fracs = {k: float(v[1]) for k, v in error_maps.items()}
        self.frac_uniform = float(frac_uniform)
        first = next(iter(self.error_maps.values()))
        self.n_images, self.h, self.w = first.n_images, first.h, first.w
        for em in self.error_maps.values():
            if (em.n_images, em.h, em.w) != (self.n_images, self.h, self.w):
                raise ValueError("neuralsim_amd: the maps of one sampler share n_images and error_map_hw")

    def _split(self, n: int):
        n_uni = int(round(n * self.frac_uniform))
        rest, tot = n - n_uni, sum(self.fracs.values()) or 1.0
        parts = {k: int(round(rest * f / tot)) for k, f in self.fracs.items()}
        first = next(iter(parts))
        parts[first] += rest - sum(parts.values())
        return n_uni, parts

    def _device(self):
        return next(iter(self.error_maps.values())).error_map.device

    def _uniforms(self, n: int, u: Optional[torch.Tensor], generator=None) -> torch.Tensor:
        if u is None:
            return torch.rand([n, 4], device=self._device(), generator=generator)
        _lib.require_device(u, "u")
        if tuple(u.shape) != (n, 4) or u.dtype != torch.float32:
            raise ValueError(f"neuralsim_amd: u must be float32 [{n}, 4], got {u.dtype} {tuple(u.shape)}")
        return u.contiguous()

    def _draw(self, n: int, u: torch.Tensor, fixed: int, fidx: Optional[torch.Tensor], xy: torch.Tensor):
        n_uni, parts = self._split(n)
        if min(parts.values()) < 0:
            raise ValueError(f"neuralsim_amd: the fractions {self.fracs} leave a negative share of {n} rows")
        row0 = 0
        for j, (k, m) in enumerate(parts.items()):       # the first map's launch serves the uniform rows, too
            cnt, nu = (m + n_uni, n_uni) if j == 0 else (m, 0)
            if cnt > 0:
                cdf_img, cdf_cell = self.error_maps[k].cdfs() if m > 0 else (None, None)
                _lib.call("nsim_errmap_draw", cdf_img, cdf_cell, self.n_images, self.h, self.w, u, cnt, nu, fixed, row0, fidx, xy)
            row0 += cnt

    @torch.no_grad()
    def sample_pixel(self, num_samples: int, fi, u: Optional[torch.Tensor] = None, generator=None) -> torch.Tensor:
        """-> xy [num_samples, 2] in (0, 1) of frame ``fi``: rows [0, n_uni) uniform, then one row range per map (``_split``).
        u [num_samples, 4] float32 uniforms (column 1: cell, 2 / 3: position inside it; None: drawn here)."""
        n, fi = int(num_samples), int(fi)
        if not 0 <= fi < self.n_images:
            raise IndexError(f"neuralsim_amd: frame {fi} outside [0, {self.n_images})")
        u = self._uniforms(n, u, generator)
        xy = torch.empty([n, 2], dtype=torch.float32, device=u.device)
        self._draw(n, u, fi, None, xy)
        return xy

    @torch.no_grad()
    def sample_img_pixel(self, num_samples: int, u: Optional[torch.Tensor] = None, generator=None):
        """-> (frame [num_samples] int64, xy [num_samples, 2]) drawn jointly over all images; u as in ``sample_pixel`` with column 0
        choosing the image."""
        n = int(num_samples)
        u = self._uniforms(n, u, generator)
        fidx = torch.empty([n], dtype=torch.long, device=u.device)
        xy = torch.empty([n, 2], dtype=torch.float32, device=u.device)
        self._draw(n, u, -1, fidx, xy)
        return fidx, xy

    def get_pdf_image(self) -> torch.Tensor:
        return torch.stack([em.get_pdf_image() * self.fracs[k] for k, em in self.error_maps.items()]).sum(0)
