"""Float64 restatement of SSIM and S3IM, written from the formulas -- the checker of tests/test_s3im.py.

SSIM of x, y [B,C,H,W]: window g2 = g g^T with g[i] ~ exp(-(i - k//2)^2 / (2 1.5^2)), i = 0..k-1, normalised to sum 1 (for an even k
the centre is off-middle); zero padding p = (k - 1) // 2, stride s, per channel;
    mu1 = g2 * x, mu2 = g2 * y, s11 = g2 * x^2 - mu1^2, s22 = g2 * y^2 - mu2^2, s12 = g2 * (x y) - mu1 mu2,
    map = (2 mu1 mu2 + C1) (2 s12 + C2) / ((mu1^2 + mu2^2 + C1) (s11 + s22 + C2)),  C1 = 0.01^2, C2 = 0.03^2,
and the mean of the map over all B C Ho Wo windows, Ho = (H + 2p - k) // s + 1.
S3IM: the virtual image [1, 3, patch_h, patch_w * R] whose pixel (i, j) is row index[i * Wv + j] of pred[:P] / gt[:P]."""
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_1d(k: int) -> torch.Tensor:
    i = torch.arange(k, dtype=torch.float64)
    g = torch.exp(-(i - k // 2) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def ssim_map(x: torch.Tensor, y: torch.Tensor, k: int, s: int) -> torch.Tensor:
    x, y = x.double(), y.double()
    C = x.shape[1]
    g = window_1d(k)
    g2 = (g[:, None] * g[None, :]).expand(C, 1, k, k).contiguous()
    p = (k - 1) // 2

    def blur(t):
        return F.conv2d(t, g2, padding=p, stride=s, groups=C)
    mu1, mu2 = blur(x), blur(y)
    s11, s22, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def ssim(x, y, k=11, s=1) -> torch.Tensor:
    return ssim_map(x, y, k, s).mean()


def virtual_image(rows: torch.Tensor, index: torch.Tensor, patch_hw) -> torch.Tensor:
    """[1, 3, patch_h, patch_w * R] from rows [N,3]: the flat sequence rows[:P][index] reshaped row-major"""
    ph, pw = patch_hw
    P = ph * pw
    return rows[:P][index].permute(1, 0).reshape(1, 3, ph, index.shape[0] // ph)


def s3im(pred, gt, index, patch_hw, k=4, s=4) -> torch.Tensor:
    """1 - SSIM of the virtual images (without the weight)"""
    return 1.0 - ssim(virtual_image(pred.double(), index, patch_hw), virtual_image(gt.double(), index, patch_hw), k, s)


def value_and_grad(fn, x, *rest, gout: float = 1.0):
    """fn(x64, *rest) and gout * d fn / d x in float64"""
    x64 = x.detach().double().requires_grad_(True)
    v = fn(x64, *rest)
    (g,) = torch.autograd.grad(v * gout, [x64])
    return v.detach(), g
