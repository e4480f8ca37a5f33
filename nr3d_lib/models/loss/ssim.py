"""``nr3d_lib.models.loss.ssim`` (app/loss/perceptual.py:60-63, 127, 142): ``ssim_module``, the mean SSIM of two image batches as an
``nn.Module``.  nr3d_lib's source is absent; the definition is that of the public pytorch-ssim / S3IM code the module wraps
(DESIGN.md sec. 7), evaluated by the fused HIP kernels of ``neuralsim_amd.losses.ssim`` -- one launch per direction instead of five
grouped ``conv2d`` and some twenty elementwise ops with their backward."""
import torch
import torch.nn as nn

from neuralsim_amd import losses as _losses

__all__ = ["ssim_module", "ssim"]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, stride: int = 1, size_average: bool = True) -> torch.Tensor:
    if not size_average:
        raise NotImplementedError("nr3d_lib.models.loss.ssim: size_average=False (a per-image SSIM) is not covered by the HIP "
                                  "kernels, which reduce over the whole batch")
    return _losses.ssim(img1, img2, window_size=window_size, stride=stride)


class ssim_module(nn.Module):
    """``ssim_module(**loss_param, device=device)`` (``PerceptualLoss(loss_type='ssim')``: window_size 11, stride 1) and
    ``ssim_module(channel=3, window_size=k, stride=s, device=device)`` (``S3IMLoss``).  ``forward(img1, img2)``: [B,C,H,W] in [0,1]
    -> 0-dim mean SSIM; gradient to ``img1`` only.  No parameters, no buffers: the window lives in the kernels."""

    def __init__(self, channel: int = 3, window_size: int = 11, stride: int = 1, size_average: bool = True, device=None, **other):
        super().__init__()
        for key in other:
            raise NotImplementedError(f"nr3d_lib.models.loss.ssim.ssim_module: option {key!r} is not covered by the HIP kernels")
        if not size_average:
            raise NotImplementedError("nr3d_lib.models.loss.ssim.ssim_module: size_average=False (a per-image SSIM) is not covered "
                                      "by the HIP kernels, which reduce over the whole batch")
        if not 1 <= int(window_size) <= _losses.SSIM_MAX_WINDOW:
            raise NotImplementedError(f"nr3d_lib.models.loss.ssim.ssim_module: window_size={window_size}: the HIP kernels take "
                                      f"windows of 1..{_losses.SSIM_MAX_WINDOW}")
        if int(stride) < 1:
            raise ValueError(f"nr3d_lib.models.loss.ssim.ssim_module: stride must be >= 1, got {stride}")
        self.channel, self.window_size, self.stride, self.size_average = int(channel), int(window_size), int(stride), True

    def forward(self, img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
        if img1.dim() != 4 or img1.shape[1] != self.channel:
            raise ValueError(f"ssim_module(channel={self.channel}) takes [B,{self.channel},H,W] images, got {tuple(img1.shape)}")
        return _losses.ssim(img1, img2, window_size=self.window_size, stride=self.stride)

    def extra_repr(self) -> str:
        return f"channel={self.channel}, window_size={self.window_size}, stride={self.stride}"
