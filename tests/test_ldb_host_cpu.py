"""dlc_ldb_describe_u8's kernel text on the host (no GPU): csrc/ldb.hip compiled as C++ against the stand-in of
tests/host_sanitize/ -- one host thread per GPU thread, barriers, shuffles and the ballot emulated -- and run as a
stand-alone program under AddressSanitizer + UBSan.  The driver holds the expected bytes as data: this file computes them
with tests/ldb_oracle.py from the driver's own generator, `python tests/test_ldb_host_cpu.py --write` prints them into
the driver, and the test refuses a driver whose block is not what the oracle gives today."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldb_oracle  # noqa: E402

DRIVER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_sanitize", "ldb", "driver.cpp")
CASES = [(2, 37, 53, 12, 12, (2, 3)), (2, 16, 16, 16, 16, (2, 4, 8))]        # the driver's `cases`
BEGIN, END = "// ---- expected: begin (generated, do not edit) ----\n", "// ---- expected: end ----\n"


def lcg_bytes(seed, n):
    """The driver's generator: s = s * 6364136223846793005 + 1442695040888963407 mod 2^64, value (s >> 33) % 256."""
    s, out = seed, np.empty(n, np.uint8)
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        out[i] = (s >> 33) % 256
    return out


def expected_block():
    lines, sizes = [], []
    for ci, (frames, hh, ww, h, w, levels) in enumerate(CASES):
        gray = lcg_bytes(ci + 1, frames * hh * ww).reshape(frames, hh, ww)
        rows = ldb_oracle.describe(gray, (h, w), levels)
        sizes.append(rows.shape[1])
        flat = ["0x%02x" % v for v in rows.reshape(-1)]
        body = ",\n".join("    " + ", ".join(flat[i:i + 16]) for i in range(0, len(flat), 16))
        lines.append("static const unsigned char expected_%d[] = {\n%s};\n" % (ci, body))
    return "static const int expected_row_bytes[] = {%s};\n" % ", ".join(str(v) for v in sizes) + "".join(lines)


def driver_parts():
    text = open(DRIVER).read()
    a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
    return text[:a], text[a:b], text[b:]


def test_driver_declares_the_cases_of_this_file():
    text = open(DRIVER).read()
    for frames, hh, ww, h, w, levels in CASES:
        decl = "{%d, %d, %d, %d, %d, %d, {%s}}" % (frames, hh, ww, h, w, len(levels), ", ".join(str(g) for g in levels))
        assert decl in text, decl


def test_expected_bytes_are_the_oracles():
    assert driver_parts()[1] == expected_block(), "run `python tests/test_ldb_host_cpu.py --write`"


def test_kernel_text_on_the_host_under_sanitizers(tmp_path):
    import host_kernel
    res = host_kernel.run(tmp_path, "ldb", "ldb")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "2 cases, 0 bad" in res.stdout
    assert not re.search(r"runtime error|AddressSanitizer", res.stderr), res.stderr[-2000:]


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    head, _, tail = driver_parts()
    open(DRIVER, "w").write(head + expected_block() + tail)
