#!/usr/bin/env python3
"""Check the gfx950 code objects of a built library for the store-data hazard of wide stores ("A store-data hazard
the ISA manual says does not exist").

A store of more than 64 bits must not be followed at once by a vector instruction that writes its data registers.  The compiler's
hazard recogniser pads that slot for buffer stores only when their scalar offset field holds no register; with an SGPR there it
inserts nothing, and gfx950 then corrupts store data under load.  binarise.hip keeps that field 0, which only holds for as long as
the compiler keeps doing so.  Rules, over every buffer_/global_/flat_/scratch_ store of dwordx3 / dwordx4:

  (a) a buffer store's soffset operand is the literal 0                                               (fails)
  (b) the next instruction is not a VALU instruction that writes one of the store's data registers   (fails)
  (c) no non-VALU instruction (a load, say) writes a data register within the next two instructions   (reported only)

    python tools/check_store_hazard.py opencv-ar_amd/lib/libocvar_hip.so      (exit 1 on a violation of (a) or (b))
"""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from dataclasses import dataclass, field

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = "gfx950"
WIDE_STORE = re.compile(r"^(buffer|global|flat|scratch)_store_dwordx[34]$")
REG = re.compile(r"^([va])(?:\[(\d+):(\d+)\]|(\d+))$")
LABEL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def regs(op):
    """the vector registers an operand names: {('v', 7)}, {('v', 64), ..., ('v', 67)}; empty for SGPRs, constants, off"""
    m = REG.match(op.strip())
    if not m:
        return set()
    lo, hi = (int(m.group(2)), int(m.group(3))) if m.group(2) else (int(m.group(4)), int(m.group(4)))
    return {(m.group(1), r) for r in range(lo, hi + 1)}


@dataclass
class Insn:
    func: str
    line: str
    mnemonic: str
    operands: list


def parse(listing):
    """llvm-objdump -d output -> instructions with their enclosing symbol; labels, blank lines and comments dropped"""
    out, func = [], "?"
    for raw in listing.splitlines():
        s = raw.strip()
        m = LABEL.match(s)
        if m:
            func = m.group(1)
            continue
        s = s.split("//")[0].strip()
        if not s or s.endswith(":") or s.startswith(";"):
            continue
        parts = s.split(None, 1)
        ops = []
        if len(parts) > 1:
            ops = [o.strip() for o in parts[1].split(",")]
            ops[-1] = ops[-1].split()[0] if ops[-1] else ops[-1]   # "0 offen nt" -> "0": modifiers follow the last operand
        out.append(Insn(func, s, parts[0], ops))
    return out


def store_data(insn):
    """a wide store's data registers: buffer_* puts vdata first, global_/flat_/scratch_ put the address first and vdata second"""
    return regs(insn.operands[0] if insn.mnemonic.startswith("buffer_") else insn.operands[1])


def written(insn):
    """vector registers an instruction writes, as far as the hazard needs: the destination operand of VALU instructions and of
    loads / LDS reads / returning atomics (v_swap writes both operands); stores write none"""
    mn = insn.mnemonic
    if not insn.operands:
        return set()
    if mn.startswith("v_swap"):
        return regs(insn.operands[0]) | regs(insn.operands[1])
    if mn.startswith("v_"):
        return regs(insn.operands[0])
    if "_store" in mn or mn.startswith("ds_write") or mn.startswith("ds_store") or mn.startswith("s_"):
        return set()
    if "_load" in mn or mn.startswith("ds_read") or mn.startswith("ds_load"):
        return regs(insn.operands[0])
    if "atomic" in mn and re.search(r"\b(glc|sc0)\b", insn.line):
        return regs(insn.operands[0])
    return set()


@dataclass
class Report:
    stores: int = 0
    per_mnemonic: Counter = field(default_factory=Counter)   # "buffer_store_dwordx4 in ocvar::binarise_crops_kernel(...)" -> count
    failures: list = field(default_factory=list)
    notes: list = field(default_factory=list)


def check_listing(listing, report=None):
    report = report or Report()
    ins = parse(listing)
    for i, st in enumerate(ins):
        if not WIDE_STORE.match(st.mnemonic):
            continue
        report.stores += 1
        report.per_mnemonic[f"{st.mnemonic} in {st.func}"] += 1
        data = store_data(st)
        if st.mnemonic.startswith("buffer_") and st.operands[3] != "0":
            report.failures.append(f"(a) soffset {st.operands[3]!r}, not 0, in {st.func}: {st.line}")
        for d, nxt in enumerate(ins[i + 1:i + 3], 1):
            hit = written(nxt) & data
            if not hit:
                continue
            if nxt.mnemonic.startswith("v_"):
                if d == 1:
                    report.failures.append(f"(b) the next VALU instruction writes store data in {st.func}: {st.line}  ->  {nxt.line}")
            else:
                report.notes.append(f"(c) instruction {d} after the store writes store data in {st.func}: {st.line}  ->  {nxt.line}")
    return report


def code_objects(so_path, workdir):
    """unbundle the library's gfx950 code objects into workdir (llvm-objdump --offloading writes next to its input)"""
    copy = os.path.join(workdir, "lib.so")
    with open(so_path, "rb") as a, open(copy, "wb") as b:
        b.write(a.read())
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, stdout=subprocess.DEVNULL, cwd=workdir)
    return sorted(os.path.join(workdir, f) for f in os.listdir(workdir) if f.endswith("--" + ARCH))


def kernel_resources(co_path):
    """{kernel symbol: {vgpr_count, vgpr_spill_count, sgpr_spill_count}} from the code object's metadata note"""
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co_path], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("  - ."):
            cur = {}
        m = re.match(r"^(?:  - |    )\.(\w+):\s+(\S+)", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                out[m.group(2)] = cur
    return {k: {f: v.get(f) for f in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count")} for k, v in out.items()}


def check_library(so_path):
    report = Report()
    with tempfile.TemporaryDirectory() as tmp:
        cos = code_objects(so_path, tmp)
        if not cos:
            raise RuntimeError(f"no {ARCH} code object in {so_path}")
        for co in cos:
            listing = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "-C", "--no-show-raw-insn", f"--mcpu={ARCH}", co],
                                     check=True, capture_output=True, text=True).stdout
            check_listing(listing, report)
            for name, res in kernel_resources(co).items():
                if "binarise" in name:
                    report.notes.append(f"resources {name}: {res}")
        report.notes.append(f"{len(cos)} code objects")
    return report


def compiler_version():
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    try:
        return subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip()
    except OSError as e:
        return f"hipcc --version: {e}"


def main(argv):
    if len(argv) != 2:
        print(__doc__.strip().splitlines()[-1].strip(), file=sys.stderr)
        return 2
    report = check_library(argv[1])
    print(compiler_version())
    for n in report.notes:
        print("note:", n)
    for f in report.failures:
        print("FAIL:", f)
    print(f"{report.stores} stores wider than 64 bits, {len(report.failures)} violations")
    return 1 if report.failures else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
