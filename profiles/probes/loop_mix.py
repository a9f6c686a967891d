"""Instruction mix of the main loop of the MFMA tile kernels, read off the compiler's assembly (no GPU needed).

conv_tiles.hip is compiled to gfx950 assembly with the build's own flags (ditreeonlineplanner_amd/build.py).  For every
kernel whose demangled name contains the given patterns the main loop (the label-to-last-backward-branch range with the
most MFMAs, then the most instructions) is counted by generic instruction class:
    MFMA (v_mfma*), other VALU (v_*), SALU (s_*, with s_waitcnt listed apart), LDS (ds_*, and how many carry an immediate
    offset), buffer (buffer_*), plus VGPRs, spilled VGPRs and scratch bytes from the kernel's metadata.
A loop unrolled over two chunks shows twice the MFMAs of one chunk: compare the per-100-MFMA columns.

    python profiles/probes/loop_mix.py                       # the halo, gemm16 and small-Conv2d kernels
    python profiles/probes/loop_mix.py conv3_halo16x3_kernel '<1, false, false, 5'
    python profiles/probes/loop_mix.py --asm out.s ...       # count an assembly file made earlier
    python profiles/probes/loop_mix.py --keep out.s ...      # keep the assembly
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from ditreeonlineplanner_amd import build as B  # noqa: E402

DEFAULT = ["conv3_halo16x3_kernel", "conv3_halo16_kernel", "gemm16_kernel", "conv2d_small_kernel"]


def compile_asm(out, defines=()):
    extra = dict(B.UNITS)["conv_tiles.hip"]
    cmd = [B.HIPCC, *B.COMMON, *extra, *defines, "--cuda-device-only", "-S", os.path.join(B.CSRC, "conv_tiles.hip"), "-o", out]
    subprocess.check_call(cmd)


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt is None:
        raise SystemExit("loop_mix: needs llvm-cxxfilt or c++filt on PATH to name the template instantiations")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels_of(text):
    """-> {symbol: list of body lines} for every .amdhsa_kernel of the file, and {symbol: metadata dict}."""
    lines = text.split("\n")
    syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    bodies = {}
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\w+):", ln)
        if m:
            start.setdefault(m.group(1), i)
    for s in syms:
        if s not in start:
            continue
        a = start[s]
        b = a
        while b < len(lines) and not lines[b].lstrip().startswith("s_endpgm"):
            b += 1
        bodies[s] = lines[a + 1:b + 1]
    meta = {}
    cur = None
    for ln in lines:
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if ln.lstrip().startswith("- .") and k in ("agpr_count", "args"):     # first key of a kernel record
            cur = {}
        if cur is not None:
            cur[k] = v
            if k == "name" and v in bodies:
                meta[v] = cur
    return bodies, meta


def insn(ln):
    s = ln.split(";")[0].strip()
    if not s or s.startswith(".") or s.endswith(":"):
        return None
    return s


def largest_loop(body):
    label_at = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            label_at[m.group(1)] = i
    last_back = {}
    for i, ln in enumerate(body):
        s = insn(ln)
        if s and (s.startswith("s_cbranch") or s.startswith("s_branch")):
            tgt = s.split()[-1]
            if tgt in label_at and label_at[tgt] < i:
                last_back[tgt] = i
    best = None
    for tgt, i in last_back.items():
        ins = [s for s in map(insn, body[label_at[tgt]:i + 1]) if s]
        key = (sum(s.startswith("v_mfma") for s in ins), len(ins))       # the K loop: most MFMAs, then most instructions
        if best is None or key > best[0]:
            best = (key, label_at[tgt], i)
    return best


def count(lines):
    c = dict(mfma=0, valu=0, salu=0, waitcnt=0, lds=0, lds_imm=0, buffer=0, other=0, valu_ops={}, salu_ops={})
    for ln in lines:
        s = insn(ln)
        if not s:
            continue
        op = s.split()[0]
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["valu_ops"][op] = c["valu_ops"].get(op, 0) + 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
            c["salu_ops"][op] = c["salu_ops"].get(op, 0) + 1
        elif op.startswith("ds_"):
            c["lds"] += 1
            c["lds_imm"] += "offset:" in s
        elif op.startswith("buffer_"):
            c["buffer"] += 1
        else:
            c["other"] += 1
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("patterns", nargs="*", help="substrings of the demangled kernel name (all given ones must match)")
    ap.add_argument("--asm", help="count this assembly file instead of compiling")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("-D", action="append", default=[], help="extra define for the compile (diagnostic builds)")
    ap.add_argument("--ops", action="store_true", help="list the VALU / SALU opcodes of each loop")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(prefix="loop_mix_"), "conv_tiles.s")
        compile_asm(path, ["-D" + d for d in args.D])
    with open(path) as f:
        bodies, meta = kernels_of(f.read())
    names = demangle(list(bodies))
    pats = args.patterns
    print(f"{'kernel':<58s} {'MFMA':>5s} {'VALU':>5s} {'SALU':>5s} {'wait':>5s} {'LDS':>4s} {'+imm':>4s} {'buf':>4s} "
          f"{'VALU/100':>8s} {'SALU/100':>8s} {'VGPR':>5s} {'spill':>5s} {'scratch':>7s}")
    for sym in sorted(bodies, key=lambda s: names[s]):
        nm = re.sub(r"^void |\(ConvGemmParams\)$", "", names[sym])
        if pats and not all(p in nm for p in pats):
            continue
        if not pats and not any(nm.startswith(d + "<") for d in DEFAULT):
            continue
        lp = largest_loop(bodies[sym])
        if lp is None:
            print(f"{nm:<58s} (no loop)")
            continue
        c = count(bodies[sym][lp[1]:lp[2] + 1])
        m = meta.get(sym, {})
        per = 100.0 / max(c["mfma"], 1)
        print(f"{nm:<58s} {c['mfma']:5d} {c['valu']:5d} {c['salu']:5d} {c['waitcnt']:5d} {c['lds']:4d} {c['lds_imm']:4d} "
              f"{c['buffer']:4d} {c['valu'] * per:8.1f} {c['salu'] * per:8.1f} {m.get('vgpr_count', '?'):>5s} "
              f"{m.get('vgpr_spill_count', '?'):>5s} {m.get('private_segment_fixed_size', '?'):>7s}")
        if args.ops:
            for kind in ("valu_ops", "salu_ops"):
                print("    " + kind[:4] + ": " + ", ".join(f"{n} {k}" for k, n in sorted(c[kind].items(), key=lambda kv: -kv[1])))


if __name__ == "__main__":
    main()
