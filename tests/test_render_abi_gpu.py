"""MI355X: tests/abi_c/render_client.cpp -- fdm_render_create -> fdm_render_forward with no Python in the process; the face-id image is
checked in the program against the integer coverage rule of include/fdm_hip.h computed there."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_c_client_renders_a_frame_without_python(tmp_path):
    from fdm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "render_client")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", os.path.join(root, "tests", "abi_c", "render_client.cpp"),
           "-I", os.path.join(root, "include"), "-L", libdir, "-lfdm_hip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "render_client ok" in r.stdout
    print(r.stdout.strip())
