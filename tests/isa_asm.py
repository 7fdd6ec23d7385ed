"""gfx950 assembly of one translation unit and the assembler's own per-kernel summary, for the register-budget
tests (tests/test_isa_guard.py and the *_abi.py modules).  Assembly is cached under build/isa/ by source + header
+ compiler hash, so only the first run after a change pays for hipcc."""
import hashlib
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr_amd", "csrc")


def _stamp():
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".h"):
            h.update(open(os.path.join(CSRC, f), "rb").read())
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    h.update(subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.encode())
    return h.hexdigest()[:16]


def _asm(path, stamp):
    """gfx950 assembly of one translation unit (cached)"""
    key = stamp + hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    cache = os.path.join(ROOT, "build", "isa")
    os.makedirs(cache, exist_ok=True)
    out = os.path.join(cache, os.path.basename(path).replace(".hip", "") + "_" + key + ".s")
    if not os.path.exists(out):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        tmp = out + ".tmp%d" % os.getpid()
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-o", tmp, path], check=True, stderr=subprocess.DEVNULL)
        os.replace(tmp, out)
    return out


def _kernel_info(asm_path):
    """{mangled name: {vgprs, scratch, occupancy, vgpr_spill, sgpr_spill}} from the assembler's own summary"""
    text = open(asm_path).read()
    info = {}
    for m in re.finditer(r"^(_Z\w+):.*?; Kernel info:(.*?); Occupancy: (\d+)", text, re.S | re.M):
        body = m.group(2)
        g = lambda k: int(re.search(r"; %s: (\d+)" % k, body).group(1))
        info[m.group(1)] = {"vgprs": g("NumVgprs"), "agprs": g("NumAgprs"), "scratch": g("ScratchSize"),
                            "occupancy": int(m.group(3))}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", text, re.S):
        d = info.setdefault(m.group(1), {})
        for key in ("vgpr_spill_count", "sgpr_spill_count"):
            mm = re.search(r"\.%s:\s+(\d+)" % key, m.group(2))
            d[key] = int(mm.group(1)) if mm else 0
    return info
