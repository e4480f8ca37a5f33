"""Generate tests/golden/s3im_fixture.pt: what the REFERENCE's own ``S3IMLoss`` and ``PerceptualLoss(loss_type='ssim')``
(app/loss/perceptual.py, loaded unchanged by tests/ref_glue.py) return on the inputs of tests/test_s3im.py -- this package's
``ssim_module`` on the emulator backend underneath -- together with everything the run drew: the inputs, the index of the virtual
image, both losses and their gradients with respect to ``rgb_volume``.  Data only.  The replay (tests/test_s3im.py::
test_reference_run_replayed_from_the_fixture) runs on both backends where the reference tree is absent.

Where the reference tree is readable:   python tests/golden/make_s3im_fixture.py"""
import ctypes
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]

import build_emu  # noqa: E402
import test_s3im as t  # noqa: E402
from neuralsim_amd import _lib  # noqa: E402


def main():
    lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
    _lib.get_lib, _lib.stream_handle, _lib.require_device = (lambda: lib), (lambda: 0), (lambda t, name="tensor": None)
    out = t.run_reference_losses(torch.device("cpu"))
    fx = dict(t.reference_inputs(), index=t.reference_index(), patch_hw=(t.S3IM_CFG["patch_height"], t.S3IM_CFG["patch_width"]),
              kernel_size=t.S3IM_CFG["kernel_size"], stride=t.S3IM_CFG["stride"], s3im_w=t.S3IM_CFG["w"], perceptual_w=t.PERC_W,
              s3im_loss=out["s3im"][0], s3im_grad=out["s3im"][1], perceptual_loss=out["perceptual"][0],
              perceptual_grad=out["perceptual"][1])
    torch.save(fx, HERE / "s3im_fixture.pt")
    print("s3im", float(fx["s3im_loss"]), "perceptual", float(fx["perceptual_loss"]), "bytes", (HERE / "s3im_fixture.pt").stat().st_size)


if __name__ == "__main__":
    main()
