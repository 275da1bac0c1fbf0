"""The kernel text of csrc/pca.hip on the host (no GPU): compiled as C++ against the stand-in of tests/host_sanitize/
-- one host thread per GPU thread, barriers emulated -- and run as a stand-alone program under AddressSanitizer + UBSan
against per-element loops over the definition of include/dlc.h: both plans and AUTO, both basis dtypes, every combination
of NULL / given mean and scale bit for bit, untouched words against a sentinel, the refusals writing nothing, every
access of the kernels a checked access."""
import host_kernel


def test_pca_kernel_text_on_the_host_under_sanitizers(tmp_path):
    res = host_kernel.run(tmp_path, "pca", "pca")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "172 cases, 0 bad" in res.stdout
