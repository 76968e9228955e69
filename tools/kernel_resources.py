"""Registers, LDS and scratch of every kernel in the built objects (csrc/_obj/*.o), one line per kernel:

    python tools/kernel_resources.py [--match REGEX] [obj_dir] > resources.txt

Reads the AMDGPU metadata note of each object's gfx950 code object (clang-offload-bundler + llvm-readelf from the ROCm LLVM).
waves/SIMD is derived from the allocated vector registers (512 per SIMD lane in granules of 8, at most 8 waves), not measured."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels_of(obj):
    with tempfile.TemporaryDirectory() as tmp:
        co, fb = os.path.join(tmp, "co"), os.path.join(tmp, "fatbin")
        if subprocess.call([os.path.join(LLVM, "llvm-objcopy"), f"--dump-section=.hip_fatbin={fb}", obj, os.path.join(tmp, "unused.o")],
                           stderr=subprocess.DEVNULL):
            return []        # a host-only unit
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", f"--input={fb}",
                               f"--targets={TARGET}", f"--output={co}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur = [], {}
    for line in notes.splitlines():
        # a kernel's own fields sit at the list item's indent ("  - .agpr_count:" opens it, "    .name:" ...); argument fields are deeper
        m = re.match(r"(  - | {4})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(2), m.group(3).strip().strip("'")
        if m.group(1) == "  - " and cur.get("name"):
            out.append(cur)
            cur = {}
        cur[k] = v
    if cur.get("name"):
        out.append(cur)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj_dir", nargs="?", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "face-diffusion-model_amd", "csrc", "_obj"))
    ap.add_argument("--match", default=".")
    a = ap.parse_args()
    rows = []
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)      # (mangled names when neither is there)
    for f in sorted(os.listdir(a.obj_dir)):
        if not f.endswith(".o"):
            continue
        for k in kernels_of(os.path.join(a.obj_dir, f)):
            name = subprocess.run([filt, k["name"]], capture_output=True, text=True).stdout.strip() if filt else k["name"]
            if not re.search(a.match, name):
                continue
            v = int(k.get("vgpr_count", 0))
            waves = min(8, 512 // max(8, -(-v // 8) * 8))
            rows.append(f"{f}\t{name}\tvgpr {v}\tagpr {k.get('agpr_count', '0')}\tsgpr {k.get('sgpr_count', '0')}\tlds {k.get('group_segment_fixed_size', '0')}"
                        f"\tscratch {k.get('private_segment_fixed_size', '0')}\twaves/SIMD {waves}")
    sys.stdout.write("\n".join(sorted(rows)) + "\n")


if __name__ == "__main__":
    main()
