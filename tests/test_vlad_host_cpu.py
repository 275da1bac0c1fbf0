"""The kernel text of csrc/vlad.hip on the host (no GPU): compiled as C++ against the stand-in of tests/host_sanitize/
-- one host thread per GPU thread, barriers emulated -- and run as a stand-alone program under AddressSanitizer + UBSan
against per-element loops over the definition of include/dlc.h and a recursive TREE: assignments, both norms of the
encoder and the k-means step bit for bit, untouched words against a sentinel, every access of the kernels a checked
access."""
import host_kernel


def test_vlad_kernel_text_on_the_host_under_sanitizers(tmp_path):
    res = host_kernel.run(tmp_path, "vlad", "vlad")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "39 cases, 0 bad" in res.stdout
