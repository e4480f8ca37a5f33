#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 device code of two source trees (a refactor must not change it).

    python tools/isa_diff.py OLD_CSRC NEW_CSRC [--jobs 16] > profiles/<record>.txt

OLD_CSRC / NEW_CSRC: two ``neuralsim_amd/csrc`` directories (e.g. an export of the parent commit and the working tree).
Every ``*.hip`` in them is compiled to device assembly with the flags of that tree's own ``build.py`` into
``<dir>/_build/isa/`` (kept: a second run only recompiles what is missing), or, if the directory holds ``*.s``
files already, those are read as they are.  Runs without a GPU.

One line per kernel symbol: ``same | changed | removed | added``, then the resource figures of the new build
(old -> new where they differ): VGPRs, AGPRs, SGPRs, spilled VGPRs / SGPRs, static LDS bytes, scratch bytes,
waves per SIMD.  ``same`` / ``changed`` is about the instruction text (local labels renumbered, comments
stripped, the kernel's own name masked).  Exit status 1 if a kernel was added or a resource got worse (more registers, spills, LDS or
scratch, fewer waves), else 0.
"""
import argparse
import importlib.util
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

FIGS = ["vgpr", "agpr", "sgpr", "vspill", "sspill", "lds", "scratch", "occ"]
COMMENT_KEYS = {"NumVgprs": "vgpr", "NumAgprs": "agpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch",
                "Occupancy": "occ", "LDSByteSize": "lds"}


def flags_of(csrc: Path):
    spec = importlib.util.spec_from_file_location("_nsim_build_flags", csrc / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod._hipcc(), list(mod.HIPCC_FLAGS)


def assembly(csrc: Path, jobs: int):
    ready = sorted(csrc.glob("*.s"))
    if ready:
        return ready
    hipcc, flags = flags_of(csrc)
    out = csrc / "_build" / "isa"
    out.mkdir(parents=True, exist_ok=True)

    def one(src):
        dst = out / (src.name + ".s")
        if not dst.exists() or dst.stat().st_mtime < max(p.stat().st_mtime for p in [src, *csrc.glob("*.h")]):
            subprocess.check_call([hipcc, *flags, "--cuda-device-only", "-S", str(src), "-o", str(dst)])
        return dst

    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(one, sorted(csrc.glob("*.hip"))))


def kernels_of(path: Path):
    """{symbol: (instruction text, {figure: value})} of one assembly file"""
    lines = path.read_text().splitlines()
    spills = {}      # per entry of the amdhsa.kernels metadata list (an entry starts at "  - ."): its .symbol and spill counts
    entry = {}
    for ln in lines + ["  - .end"]:
        if re.match(r"\s+- \.", ln) and not ln.startswith("      "):
            if "symbol" in entry:
                spills[entry["symbol"]] = (entry.get("vgpr_spill_count", 0), entry.get("sgpr_spill_count", 0))
            entry = {}
        if m := re.match(r"\s+(?:- )?\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", ln):
            entry[m.group(1)] = int(m.group(2))
        elif m := re.match(r"\s+(?:- )?\.symbol:\s+(\S+)\.kd", ln):
            entry["symbol"] = m.group(1)
    out = {}
    for name in spills:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text = []
        for ln in lines[start + 1:end]:
            ln = re.sub(r"\.L(BB|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), ln.split(";")[0]).strip()
            ln = ln.replace(name, "<kernel>")      # (directives name the kernel itself; --map may have renamed it)
            if ln and not ln.startswith((".section", ".text")):      # (a template kernel sits in a COMDAT section, a plain one in .text)
                text.append(ln)
        figs = dict.fromkeys(FIGS, 0)
        for ln in lines[end:end + 60]:      # the "; Kernel info:" block behind the function
            if m := re.match(r";\s*(\w+):\s*(\d+)", ln):
                if m.group(1) in COMMENT_KEYS:
                    figs[COMMENT_KEYS[m.group(1)]] = int(m.group(2))
            elif ln.startswith("\t.text"):
                break
        figs["vspill"], figs["sspill"] = spills[name]
        out[name] = ("\n".join(text), figs)
    return out


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, res.stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite the old build's demangled names (a kernel that lost a constant template parameter)")
    args = ap.parse_args()
    sides = []
    for d in (args.old, args.new):
        ks = {}
        for s in assembly(d, min(args.jobs, 16)):
            ks.update(kernels_of(s))
        sides.append(ks)
    pretty = demangle(sorted(set(sides[0]) | set(sides[1])))
    old, new = ({pretty[n]: v for n, v in ks.items()} for ks in sides)
    for m in args.map:
        pat, repl = m.split("=", 1)
        old = {re.sub(pat, repl, n): v for n, v in old.items()}
    bad = 0
    count = dict.fromkeys(["same", "changed", "removed", "added"], 0)
    for name in sorted(set(old) | set(new)):
        if name not in new:
            state, figs, was = "removed", old[name][1], old[name][1]
        elif name not in old:
            state, figs, was = "added", new[name][1], new[name][1]
            bad = 1
        else:
            state = "same" if old[name][0] == new[name][0] else "changed"
            figs, was = new[name][1], old[name][1]
        count[state] += 1
        cols = []
        for f in FIGS:
            cols.append(f"{f}={figs[f]}" if was[f] == figs[f] else f"{f}={was[f]}->{figs[f]}")
            worse = figs[f] < was[f] if f == "occ" else figs[f] > was[f]
            if worse:
                bad = 1
                cols[-1] += "(!)"
        print(f"{name.removeprefix('void ').replace('(FieldArgs)', '')}  {state}  " + " ".join(cols))
    print("# " + ", ".join(f"{v} {k}" for k, v in count.items()) + (": REGRESSION" if bad else ": ok"))
    return bad


if __name__ == "__main__":
    sys.exit(main())
