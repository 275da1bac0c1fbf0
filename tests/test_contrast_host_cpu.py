"""dlc_contrast_rows' kernel text on the host (no GPU): csrc/contrast_rows.hip compiled as C++ against the stand-in of
tests/host_sanitize/ -- one host thread per GPU thread, barriers emulated -- and run as a stand-alone program under
AddressSanitizer + UBSan against per-cell loops over the definition -- bit for bit, untouched words against a sentinel,
every access of the kernel a checked access."""
import host_kernel


def test_kernel_text_on_the_host_under_sanitizers(tmp_path):
    res = host_kernel.run(tmp_path, "contrast", "contrast_rows")
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "735 cases, 0 bad cells" in res.stdout
