"""Compares the gfx950 assembly of translation units between a git revision and the working tree, kernel by kernel.

    python scripts/isa_diff.py [--diff] [--mix] <base-rev> [files...]          (default: the three compositing files)

The gate of a refactor that must not change a shipped kernel: each named file of gaussian_transformer_amd/csrc is compiled to
assembly (device side only) with the flags gaussian_transformer_amd/build.py gives it -- COMMON + SOURCES[file], imported, not
copied -- once from `git show <base-rev>:...` laid out in a temporary directory (headers included) and once from the working tree.
The listings are split per function symbol and normalised (comments, .file/.loc/.ident, the __hip_cuid_<hash> symbol hipcc derives
from the source text, the function index in compiler-made labels); per kernel it prints `identical`, `reordered` or `differs` and the register,
scratch and LDS figures of the code object's metadata from both sides.  `reordered`: another text of as many instructions, with the
same multiset of mnemonics (first token of each line that is no label) and the same four figures.  Exit status 1 if any kernel
differs or exists on one side only, 0 if every kernel is identical or reordered.  --diff adds a unified diff of each kernel that differs,
--mix its instruction mix: the two instruction totals and every mnemonic whose count is not the same on both sides, with both counts.
Host-only: needs hipcc, no GPU.  It compares text; it looks for no particular instruction.
"""
from __future__ import annotations

import difflib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = "gaussian_transformer_amd/csrc"
DEFAULT_FILES = ["composite_fwd.hip", "composite_bwd.hip", "depth_maps.hip"]
FIGURES = ["vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"]

_DROP = re.compile(r"^\.(file|loc|ident|section|text|p2align|globl|weak|hidden|protected|type|size|set|addrsig\w*|cfi_\w+)\b")
_TYPE_FN = re.compile(r"^\s*\.type\s+(\S+),@function")
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:")
_LABEL_FN = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+")


def normalise_line(line: str) -> str:
    """One listing line without its comment, with canonical spacing and without the parts that depend on the source text alone."""
    line = line.split(";", 1)[0]
    line = " ".join(line.split())
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", line)
    return _LABEL_FN.sub(lambda m: ".L" + m.group(1), line)      # .LBB12_3 -> .LBB_3: the function's index in the file


def split_kernels(text: str) -> dict:
    """{symbol: {"body": [normalised lines], "figures": {name: value}}} for every function of an AMDGPU assembly listing."""
    out, name, body, in_desc = {}, None, [], False
    for raw in text.splitlines():
        m = _TYPE_FN.match(raw)
        if m:
            name, body, in_desc = m.group(1), [], False
            continue
        if name is None:
            continue
        if _FUNC_END.match(raw.strip()):
            out[name] = {"body": body, "figures": {}}
            name = None
            continue
        s = raw.strip()
        if s.startswith(".amdhsa_kernel"):        # the kernel descriptor sits inside the function's range: its figures come from the metadata
            in_desc = True
        if in_desc:
            in_desc = not s.startswith(".end_amdhsa_kernel")
            continue
        line = normalise_line(raw)
        if line and not _DROP.match(line) and line != name + ":":
            body.append(line)
    # metadata: kernel entries start at "  - .", their own keys are indented by four spaces (arguments lie deeper)
    cur = None
    for raw in text.splitlines():
        if raw.startswith("  - ."):
            cur = {}
            raw = "    " + raw[4:]
        m = re.match(r"^    \.(\w+):\s*(\S+)", raw)
        if cur is None or not m:
            continue
        cur[m.group(1)] = m.group(2)
        if "name" in cur and cur["name"] in out:
            out[cur["name"]]["figures"] = cur
    for k in out.values():
        k["figures"] = {f: k["figures"].get(f, "-") for f in FIGURES}
    return out


def _mnemonics(body):
    """The first token of every line that is no label, as a multiset"""
    return Counter(line.split()[0] for line in body if not line.endswith(":"))


def compare(base_text: str, new_text: str):
    """([(symbol, verdict, base figures or None, new figures or None)], number of symbols that are neither `identical` nor `reordered`)

    `reordered`: the bodies differ, but in as many instructions, with the same multiset of mnemonics and the same four figures -- what
    a compiler makes of the same arithmetic reached through another spelling (operands of commutative instructions swapped, registers
    renumbered, instructions scheduled in another order)."""
    base, new = split_kernels(base_text), split_kernels(new_text)
    rows, bad = [], 0
    for sym in sorted(set(base) | set(new)):
        b, n = base.get(sym), new.get(sym)
        if b is None or n is None:
            verdict = "only in base" if n is None else "only in working tree"
        elif b["body"] == n["body"]:
            verdict = "identical"
        elif b["figures"] == n["figures"] and _mnemonics(b["body"]) == _mnemonics(n["body"]):   # equal multisets: equal counts
            verdict = "reordered"
        else:
            verdict = "differs"
        bad += verdict not in ("identical", "reordered")
        rows.append((sym, verdict, b and b["figures"], n and n["figures"]))
    return rows, bad


def kernel_mix(base_text: str, new_text: str, sym: str):
    """((instructions in base, in the working tree), [(mnemonic, count in base, in the working tree)] for the unequal counts, by name)"""
    b, n = (_mnemonics(split_kernels(t)[sym]["body"]) for t in (base_text, new_text))
    return (sum(b.values()), sum(n.values())), [(m, b[m], n[m]) for m in sorted(set(b) | set(n)) if b[m] != n[m]]


def kernel_diff(base_text: str, new_text: str, sym: str) -> str:
    base, new = split_kernels(base_text), split_kernels(new_text)
    return "\n".join(difflib.unified_diff(base[sym]["body"], new[sym]["body"], "base", "working tree", lineterm="", n=2))


def _load_build():
    spec = importlib.util.spec_from_file_location("_gsr_build", os.path.join(ROOT, "gaussian_transformer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _assemble(build, tree: str, name: str, out: str) -> str:
    cmd = [build.hipcc(), "-S", "--cuda-device-only", os.path.join(tree, CSRC_REL, name), "-o", out] + build.COMMON + build.SOURCES[name]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {name} of {tree}:\n{r.stdout}\n{r.stderr}")
    with open(out) as f:
        return f.read()


def _checkout(rev: str, dest: str) -> None:
    """csrc/ and include/ of `rev`, file by file from `git show`, in the layout the sources' relative includes expect"""
    paths = subprocess.check_output(["git", "ls-tree", "-r", "--name-only", rev, "--", CSRC_REL, "include"], cwd=ROOT, text=True).split()
    for p in paths:
        os.makedirs(os.path.dirname(os.path.join(dest, p)), exist_ok=True)
        with open(os.path.join(dest, p), "wb") as f:
            f.write(subprocess.check_output(["git", "show", f"{rev}:{p}"], cwd=ROOT))


def _demangle(syms):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True)
        return dict(zip(syms, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main(argv) -> int:
    show, mix = "--diff" in argv, "--mix" in argv
    argv = [a for a in argv if a not in ("--diff", "--mix")]
    if len(argv) < 2 or argv[1].startswith("-"):
        print(__doc__)
        return 2
    rev, files = argv[1], argv[2:] or DEFAULT_FILES
    build = _load_build()
    total = bad_total = reordered_total = 0
    with tempfile.TemporaryDirectory() as tmp:
        _checkout(rev, os.path.join(tmp, "base"))
        jobs = [(os.path.join(tmp, "base"), f, os.path.join(tmp, "base_" + f + ".s")) for f in files] + \
               [(ROOT, f, os.path.join(tmp, "new_" + f + ".s")) for f in files]
        with ThreadPoolExecutor(max_workers=4) as ex:
            texts = list(ex.map(lambda j: _assemble(build, *j), jobs))
    for i, f in enumerate(files):
        rows, bad = compare(texts[i], texts[len(files) + i])
        names = _demangle([r[0] for r in rows])
        print(f"== {f} ({' '.join(build.COMMON + build.SOURCES[f])}): {len(rows)} functions, {bad} neither identical nor reordered")
        for sym, verdict, b, n in rows:
            fig = " ".join(f"{k.split('_')[0]}={(b or {}).get(k, '-')}/{(n or {}).get(k, '-')}" for k in FIGURES)
            print(f"{verdict:21s} {fig:44s} {names[sym]}")
            if mix and verdict == "differs":
                (tb, tn), rows_m = kernel_mix(texts[i], texts[len(files) + i], sym)
                print(f"    instructions {tb}/{tn}; unequal counts: " + "  ".join(f"{m} {cb}/{cn}" for m, cb, cn in rows_m))
            if show and verdict == "differs":
                print(kernel_diff(texts[i], texts[len(files) + i], sym))
        total += len(rows)
        bad_total += bad
        reordered_total += sum(r[1] == "reordered" for r in rows)
    print(f"== total: {total} functions against {rev}, {total - bad_total - reordered_total} identical, {reordered_total} reordered, "
          f"{bad_total} differing or one-sided   (figures: base/working tree; vgpr, sgpr, private = scratch bytes, group = LDS bytes)")
    return 1 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
