"""One build-and-run recipe for the kernel texts that run on the host (tests/test_{contrast,fuse,vlad,pca}_host_cpu.py):
a kernel's .hip is compiled as C++ in front of tests/host_sanitize/<name>/driver.cpp, against the shared stand-in
tests/host_sanitize/dlc_internal.h and the library's own include/dlc.h, csrc/dlc_hd.h, csrc/entry.h, csrc/lds_tree.h and
csrc/score_rows.h, and run as a stand-alone program under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # the vector types of the kernel texts are clang's (the compiler hipcc drives)
FLAGS = ["-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined"]


def run(tmp_path, name, kernel):
    """Build tests/host_sanitize/<name>/driver.cpp around csrc/<kernel>.hip in tmp_path and run it: the finished process."""
    csrc = os.path.join(ROOT, "deeploopcloser_amd", "csrc")
    san = os.path.join(ROOT, "tests", "host_sanitize")
    # the tree's own layout, so that every #include "..." finds its file as it is written; the stand-in takes the
    # place of csrc/dlc_internal.h, and csrc/score_rows.h sits beside it so that it includes the stand-in
    work = tmp_path / "deeploopcloser_amd" / "csrc"
    work.mkdir(parents=True)
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "dlc.h"), str(tmp_path / "include"))
    shutil.copy(os.path.join(csrc, kernel + ".hip"), str(work / (kernel + ".cpp")))
    for path in [os.path.join(csrc, h) for h in ("dlc_hd.h", "entry.h", "lds_tree.h", "score_rows.h")] + \
            [os.path.join(san, "dlc_internal.h"), os.path.join(san, name, "driver.cpp")]:
        shutil.copy(path, str(work))
    exe = str(work / (name + "_host"))
    subprocess.check_call([CLANG] + FLAGS + [str(work / "driver.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=600)
