"""Generate tests/golden/wpack_sha256.json: byte length and sha256 of the MFMA weight pack of every case of the
``test_*_weight_pack_bytes`` tests (tests/test_field.py, test_distant.py, test_nerf.py, test_sky.py), which own the case
lists and the metas; the masters come from ``util.det_weights`` (integer arithmetic, no RNG).

The file pins the operand format of csrc/mfma_mlp.h.  It is generated on the emulator backend (the same kernel sources
compiled for the host; the MI355X writes the same bytes).  Re-generate it only for a deliberate change of the format.  Run from the repo root:  python tests/golden/make_wpack_fixture.py
"""
import ctypes
import importlib
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tests" / "emu")]
import build_emu
from neuralsim_amd import _lib

lib = _lib.bind(ctypes.CDLL(str(build_emu.build())))
_lib.get_lib = lambda: lib
_lib.stream_handle = lambda: 0
_lib.require_device = lambda t, name="tensor": None

out = {}
for family, module in (("field", "test_field"), ("distant", "test_distant"), ("ngp", "test_nerf"), ("sky", "test_sky")):
    mod = importlib.import_module(module)
    out[family] = {case: mod.wpack_case(case, torch.device("cpu")) for case in mod.WPACK_CASES}
Path(__file__).with_name("wpack_sha256.json").write_text(json.dumps(out, indent=1) + "\n")
print("wrote wpack_sha256.json:", {k: len(v) for k, v in out.items()})
