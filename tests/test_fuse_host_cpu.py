"""dlc_fuse_rows' kernel text on the host (no GPU): csrc/fuse_rows.hip compiled as C++ against the stand-in of
tests/host_sanitize/fuse/ -- one host thread per GPU thread, barriers and shuffles emulated -- and run as a stand-alone
program under AddressSanitizer + UBSan against a recursive TREE and per-cell loops over the definition: bit for bit, both
plans, untouched words against a sentinel, every access of the kernel a checked access."""
import os
import shutil
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # the vector types of the kernel text are clang's (the compiler hipcc drives)


def test_kernel_text_on_the_host_under_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "host_sanitize", "fuse")
    shutil.copy(os.path.join(ROOT, "deeploopcloser_amd", "csrc", "fuse_rows.hip"), str(tmp_path / "fuse_rows.cpp"))
    shutil.copy(os.path.join(ROOT, "deeploopcloser_amd", "csrc", "score_rows.h"), str(tmp_path / "score_rows.h"))
    for name in ("dlc_internal.h", "driver.cpp"):
        shutil.copy(os.path.join(here, name), str(tmp_path / name))
    exe = str(tmp_path / "fuse_host")
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-g", "-w", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", str(tmp_path), str(tmp_path / "driver.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "72 cases, 0 bad" in res.stdout
