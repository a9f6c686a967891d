"""The generated K loop of the fixed-length halo kernels (conv3_halo16x3_fixed_kernel / conv3_halo16_fixed_kernel, L = 16 / 32 /
64), read off the compiler's assembly; no GPU needed.  tests/test_cabi.py guards the run-time-L kernels the same way.

  * counted waits: the loop waits for its LDS-DMA stages with s_waitcnt vmcnt(3) / vmcnt(2), which is only sound while the
    loop issues no other vector-memory operation: no scratch access (spill) and no global / flat access inside it, and
    these kernels do not spill at all;
  * the loop body is two channel chunks (the LDS buffer parity is a constant of each half): 2 x 3 K-steps x 96 (split) or
    64 (plain) MFMAs;
  * fragment addressing: at most 16 VALU instructions per chunk besides the MFMAs (the run-time form has 124) -- one XOR for
    each of the twelve lo-plane (plain: second-half) fragment reads at L = 16, none for the others.
"""
import os
import re
import subprocess

import pytest

from tests.util import REPO


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from ditreeonlineplanner_amd import build as B
    out = tmp_path_factory.mktemp("halo_fixed") / "conv_tiles.s"
    flags = list(B.COMMON) + list(dict(B.UNITS)["conv_tiles.hip"])
    subprocess.run([B.HIPCC, *flags, "--cuda-device-only", "-S", os.path.join(B.CSRC, "conv_tiles.hip"), "-o", str(out)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out.read_text()


def _mfma_loops(body):
    loops = []
    for h in [n for n, l in enumerate(body) if "Loop Header" in l]:
        label = body[h].split(":")[0].strip()
        back = [n for n, l in enumerate(body) if re.search(r"s_cbranch\w+\s+" + re.escape(label) + r"\b", l)]
        assert back, "no backward branch to a loop header"
        loops.append(body[h:back[-1] + 1])
    return [lp for lp in loops if any("v_mfma" in l for l in lp)]


CASES = [(split, et, lm) for split in (1, 0) for et in (0, 1) for lm in (16, 32, 64)]


@pytest.mark.parametrize("split,et,lm", CASES)
def test_fixed_halo_kernel_loop(asm, split, et, lm):
    name = (f"_Z27conv3_halo16x3_fixed_kernelILi{et}ELi{lm}EEv14ConvGemmParams:" if split
            else f"_Z25conv3_halo16_fixed_kernelILi{et}ELi{lm}EEv14ConvGemmParams:")
    start = asm.index(name)
    body = asm[start:asm.index(".Lfunc_end", start)].splitlines()
    assert not any("scratch_" in l for l in body), "register spills in a fixed-length halo kernel"
    loops = _mfma_loops(body)
    two_chunk = [lp for lp in loops if sum("v_mfma" in l for l in lp) == 2 * 3 * (96 if split else 64)]
    assert len(two_chunk) == 1, [sum("v_mfma" in l for l in lp) for lp in loops]
    loop = two_chunk[0]
    mfma = "f16" if et else "bf16"
    assert all(f"v_mfma_f32_16x16x32_{mfma}" in l for l in loop if "v_mfma" in l)
    assert any("vmcnt(3)" in l for l in loop) and any("vmcnt(2)" in l for l in loop)      # the counted waits of T = 0 and T = 1
    for lp in loops:                                                                      # every MFMA loop, the leftover-chunk one too
        offenders = [l.strip() for l in lp if "scratch_" in l or re.search(r"\b(global|flat)_(load|store)", l)]
        assert not offenders, offenders
    ops = [l.split(";")[0].split() for l in loop]
    valu = [o[0] for o in ops if o and o[0].startswith("v_") and not o[0].startswith("v_mfma")]
    assert len(valu) <= 2 * 16, (len(valu), sorted(set(valu)))
    assert sum(o[0] == "ds_read_b128" for o in ops if o) == 2 * 72
