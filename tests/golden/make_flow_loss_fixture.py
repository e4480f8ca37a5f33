"""Generate tests/golden/flow_loss_fixture.json: what the REFERENCE's own ``FlowLoss`` (app/loss/flow.py, loaded unchanged by
tests/ref_glue.py) returns on the cases of tests/dynamic_flow_ref.py (``FLOW_BLOCK_CASES`` on ``flow_block_inputs``) -- per case
and key the value on float64 inputs and on the float32 inputs the package sees (their difference is the reference's own rounding,
which sets the replay's bound).  Data only.  The replay (tests/test_dynamic_flow.py::test_flow_block_replayed_from_the_fixture)
runs on both backends where the reference tree is absent.

Where the reference tree is readable:   python tests/golden/make_flow_loss_fixture.py"""
import json
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import dynamic_flow_ref as fref  # noqa: E402
import ref_glue  # noqa: E402


def reference_cases():
    """case -> key -> [float64 value, float32 value]"""
    from nr3d_lib.models.annealers import get_anneal_val
    out = {}
    with ref_glue.reference_loss_module("flow") as mod:
        mod.get_anneal_val = get_anneal_val          # (the glue's stand-in is None: the annealed cases need the schedule)
        for name, (block, it) in fref.FLOW_BLOCK_CASES.items():
            r64 = fref.reference_flow_terms(mod, block, it, *fref.flow_block_inputs(torch.float64))
            r32 = fref.reference_flow_terms(mod, block, it, *fref.flow_block_inputs(torch.float32))
            assert list(r64) == list(r32)
            out[name] = {k: [float(r64[k]), float(r32[k].double())] for k in r64}
    return out


def main():
    fx = reference_cases()
    path = HERE / "flow_loss_fixture.json"
    path.write_text(json.dumps(fx, indent=1) + "\n")
    print({k: len(v) for k, v in fx.items()}, "bytes", path.stat().st_size)


if __name__ == "__main__":
    main()
