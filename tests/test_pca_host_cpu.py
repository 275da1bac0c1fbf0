"""The kernel text of csrc/pca.hip on the host (no GPU): compiled as C++ against the stand-in of tests/host_sanitize/pca/
-- one host thread per GPU thread, barriers emulated -- and run as a stand-alone program under AddressSanitizer + UBSan
against per-element loops over the definition of include/dlc.h: both plans and AUTO, both basis dtypes, every combination
of NULL / given mean and scale bit for bit, untouched words against a sentinel, the refusals writing nothing, every
access of the kernels a checked access."""
import os
import shutil
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # the compiler hipcc drives


def test_pca_kernel_text_on_the_host_under_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "host_sanitize", "pca")
    shutil.copy(os.path.join(ROOT, "deeploopcloser_amd", "csrc", "pca.hip"), str(tmp_path / "pca.cpp"))
    for name in ("dlc_internal.h", "driver.cpp"):
        shutil.copy(os.path.join(here, name), str(tmp_path / name))
    exe = str(tmp_path / "pca_host")
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-g", "-w", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", str(tmp_path), str(tmp_path / "driver.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "172 cases, 0 bad" in res.stdout
