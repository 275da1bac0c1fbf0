"""dlc_contrast_rows' kernel text on the host (no GPU): csrc/contrast_rows.hip compiled as C++ against the stand-in of
tests/host_sanitize/contrast/ and run thread by thread under AddressSanitizer + UBSan against per-cell loops over the
definition -- bit for bit, untouched words against a sentinel, every access of the kernel a checked access."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_kernel_text_on_the_host_under_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "host_sanitize", "contrast")
    shutil.copy(os.path.join(ROOT, "deeploopcloser_amd", "csrc", "contrast_rows.hip"), str(tmp_path / "contrast_rows.cpp"))
    shutil.copy(os.path.join(ROOT, "deeploopcloser_amd", "csrc", "score_rows.h"), str(tmp_path / "score_rows.h"))
    for name in ("dlc_internal.h", "driver.cpp"):
        shutil.copy(os.path.join(here, name), str(tmp_path / name))
    exe = str(tmp_path / "contrast_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-w", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", str(tmp_path), str(tmp_path / "driver.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "735 cases, 0 bad cells" in res.stdout
