"""Wave-uniformity analysis of one kernel source file, shared by the *_api.py tests.

Compiles the file to LLVM IR as scripts/uniformity_check.py compiles a kernel (headers it
includes come along by inclusion) and parses the uniformity printer's output per kernel.
"""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Instructions a wave must reach together: barriers, ballots, lane reads, shuffles, DPP.
COLLECTIVE = re.compile(r"llvm\.amdgcn\.(s\.barrier|wave\.barrier|ballot|readlane|readfirstlane|writelane|"
                        r"ds\.bpermute|ds\.permute|ds\.swizzle|update\.dpp|mov\.dpp|permlane|wave\.reduce|"
                        r"set\.inactive|icmp\.|fcmp\.)")


def analyse(src, pattern):
    """{kernel name: (blocks {label: text}, [(depth, [labels])] of the divergent-exit cycles)}
    of the kernels of `src` whose name matches `pattern`."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import uniformity_check as uc

    if not (os.path.exists(uc.HIPCC) and os.path.exists(uc.OPT)):
        pytest.skip("needs hipcc and the ROCm LLVM opt")
    with tempfile.TemporaryDirectory() as td:
        ll = os.path.join(td, "k.ll")
        subprocess.run([uc.HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-emit-llvm", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-I",
                        os.path.join(ROOT, "include"), "-o", ll, src], check=True, stdout=subprocess.DEVNULL,
                       stderr=subprocess.DEVNULL)
        r = subprocess.run([uc.OPT, "-mtriple=amdgcn-amd-amdhsa", "-mcpu=gfx950", "-passes=print<uniformity>",
                            "-disable-output", ll], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                           text=True)
        text = open(ll).read()
    # the tool's own count of each kernel's cycles must agree with the parse below
    counts = {k: len(v) for k, v in uc.divergent_exit_cycles(src, pattern, [os.path.join(ROOT, "include")]).items()}
    out = {}
    parts = re.split(r"^UniformityInfo for function '([^']+)':$", r.stderr, flags=re.M)
    for name, body in zip(parts[1::2], parts[2::2]):
        head = body.split("TEMPORAL DIVERGENCE LIST:")[0].split("\nBLOCK ")[0]
        cycles = []
        if "CYCLES WITH DIVERGENT EXIT:" in head:
            for m in re.finditer(r"^\s*depth=(\d+): entries\(([^)]*)\)([^\n]*)", head, flags=re.M):
                cycles.append((int(m.group(1)), m.group(2).split() + m.group(3).split()))
        fn = re.search(r"^define [^\n]*@" + re.escape(name) + r"\(.*?^\}", text, flags=re.S | re.M)
        assert fn, name
        blocks, label = {}, "entry"
        for line in fn.group(0).splitlines()[1:]:
            m = re.match(r"^([\w.$-]+):", line)
            if m:
                label = m.group(1)
            blocks[label] = blocks.get(label, "") + line + "\n"
        assert counts.get(name) == len(cycles), (name, counts.get(name), cycles)
        out[name] = (blocks, cycles)
    return out


def kernel(analysis, pattern):
    hits = [k for k in analysis if re.search(pattern, k)]
    assert len(hits) == 1, (pattern, hits)
    return analysis[hits[0]]


def no_collective_in(blocks, cycles):
    for depth, labels in cycles:
        for lb in labels:
            assert lb in blocks, (lb, sorted(blocks)[:8])
            assert not COLLECTIVE.search(blocks[lb]), (depth, lb, COLLECTIVE.search(blocks[lb]).group(0))
