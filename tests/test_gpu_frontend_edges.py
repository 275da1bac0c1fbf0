"""The patch front-end (csrc/frontend.hip) at the edges tests/test_frontend.py does not enter: the patch gather at every
patch size that changes its loop shape and in both output types, the grey conversion past its workgroup cap, and the
Harris selection at the lengths where its winners leave LDS.  All three are integer arithmetic or one correctly rounded
division per byte value, so every comparison is == with oracle.patches / oracle.keypoints."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import keypoints as okp
from oracle import patches as opatch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, BAD_SHAPE = 0, -1, -2
DLC_F32, DLC_F64 = 2, 3


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


# ---- patch gather ---------------------------------------------------------------------------------------------------
# 1: a single pixel; 3, 15: fewer than 256 elements; 17: just above; 41: the reference's; 45: 2025 elements, one trip of
# the eight-per-thread loop; 47: 2209, a second trip; 63; 257: wider than the workgroup
PATCH_SIZES = (1, 3, 15, 17, 41, 45, 47, 63, 257)


def edge_key_points(h, w, ps):
    """28 (x, y) centres; as in the reference the first coordinate walks image dimension 0."""
    half, far = ps // 2, 10 ** 6
    pts = [(0, 0), (h - 1, 0), (0, w - 1), (h - 1, w - 1),                                  # the corners
           (-1, w // 2), (h, w // 2), (h // 2, -1), (h // 2, w),                             # one pixel outside each edge
           (-far, w // 2), (far, w // 2), (h // 2, -far), (h // 2, far), (-far, far), (far, -far),
           (h // 2, w // 2)]
    for v in (half - 1, half, half + 1, h - half - 2, h - half - 1, h - half):                # each clamp boundary
        pts.append((v, w // 2))
    for v in (half - 1, half, half + 1, w - half - 2, w - half - 1, w - half):
        pts.append((h // 2, v))
    pts.append((half + 1, w - half - 2))
    assert len(pts) == 28
    return np.array(pts, dtype=np.int32)


def patches_model(gray, kps, ps, np_dtype):
    """oracle.patches: get_1d_boundaries' windows (vectorized_patches), then pixel / 255 in the output type."""
    f, p = kps.shape[:2]
    out = np.empty((f, p, ps * ps), dtype=np_dtype)
    for i in range(f):
        out[i] = opatch.vectorized_patches(gray[i], kps[i], ps).astype(np_dtype) / np_dtype(255)
    return out


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("ps", PATCH_SIZES)
def test_patch_gather_equals_the_oracle(eng, ps, dtype):
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    rng = np.random.RandomState(ps)
    for (h, w) in ((ps + 1, ps + 2), (ps, ps + 3), (ps + 2, ps)):       # barely larger; H == patch_size; W == patch_size
        pts = edge_key_points(h, w, ps)
        for p in (7, 1):
            kps = pts.reshape(-1, p, 2)
            gray = rng.randint(0, 256, (kps.shape[0], h, w)).astype(np.uint8)      # every frame its own content
            got = eng.extract_patches(torch.from_numpy(gray).to(eng.device), torch.from_numpy(kps).to(eng.device), ps, dtype)
            assert got.dtype == dtype and tuple(got.shape) == (kps.shape[0], p, ps * ps)
            want = patches_model(gray, kps, ps, np_dtype)
            assert want.dtype == np_dtype
            assert np.array_equal(got.cpu().numpy(), want), (ps, h, w, p)
    if ps == 41:                                                            # the model is oracle.patches.parse for fp64
        assert np.array_equal(patches_model(gray[:1], kps[:1], ps, np.float64)[0], opatch.parse(gray[0], kps[0], ps))


def test_patch_gather_refusals_write_nothing(eng):
    gray = torch.zeros((2, 40, 50), dtype=torch.uint8, device=eng.device)
    kps = torch.zeros((2, 3, 2), dtype=torch.int32, device=eng.device)
    for ps, status in ((0, BAD_ARG), (2, BAD_ARG), (40, BAD_ARG), (-1, BAD_ARG), (41, BAD_SHAPE), (51, BAD_SHAPE)):
        for dt in (DLC_F64, DLC_F32):
            out = torch.full((2 * 3 * 51 * 51,), -7.0, dtype=torch.float64, device=eng.device)
            rc = eng.lib.dlc_extract_patches(eng.ctx, C.c_void_p(gray.data_ptr()), 2, 40, 50, C.c_void_p(kps.data_ptr()), 3, ps,
                                             dt, C.c_void_p(out.data_ptr()), eng._stream())
            assert rc == status, ps
            torch.cuda.synchronize()
            assert bool((out == -7.0).all()), ps
    with pytest.raises(ValueError):
        eng.extract_patches(gray, kps, 40)


# ---- grey conversion past the workgroup cap --------------------------------------------------------------------------
def device_pixels(eng, n_bytes, seed):
    g = torch.Generator(device=eng.device)
    g.manual_seed(seed)
    return torch.randint(0, 256, (n_bytes,), generator=g, device=eng.device, dtype=torch.int32).to(torch.uint8)


def test_gray_dword_path_second_lap_and_tail(eng):
    """8192 workgroups x 256 threads x 4 pixels, three more full rows of threads and 3 pixels: the grid-stride loop goes
    round and the byte tail starts behind the last whole quad."""
    n = 8192 * 256 * 4 + 4 * 256 * 3 + 3
    rgb = device_pixels(eng, 3 * n, 21).view(n, 3)
    assert rgb.data_ptr() % 4 == 0
    got = eng.rgb_to_gray(rgb)
    assert got.data_ptr() % 4 == 0
    assert np.array_equal(got.cpu().numpy(), opatch.bgr2gray_opencv(rgb.cpu().numpy()))


def test_gray_byte_path_second_lap(eng):
    """A view 3 bytes into a buffer takes the byte path: 8192 workgroups x 256 threads and 301 pixels."""
    n = 8192 * 256 + 301
    flat = device_pixels(eng, 3 * n + 3, 22)
    view = flat[3:].view(n, 3)
    assert view.data_ptr() % 4 != 0 and view.is_contiguous()
    got = eng.rgb_to_gray(view)
    assert np.array_equal(got.cpu().numpy(), opatch.bgr2gray_opencv(view.cpu().numpy()))


# ---- Harris selection -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise_frames():
    return np.random.RandomState(96160).randint(0, 256, (3, 96, 160)).astype(np.uint8)


@pytest.mark.parametrize("n", [255, 256, 257, 512])
def test_harris_selection_at_the_flush_lengths(eng, noise_frames, n):
    """The winners wait in LDS and leave 256 at a time: n one below, at and one above a flush, and two flushes.  The same
    frames one byte into a buffer take the byte loader although W % 4 == 0."""
    f, h, w = noise_frames.shape
    assert w % 4 == 0
    aligned = torch.from_numpy(noise_frames).to(eng.device)
    buf = torch.zeros((f * h * w + 1,), dtype=torch.uint8, device=eng.device)
    buf[1:] = aligned.reshape(-1)
    shifted = buf[1:].view(f, h, w)
    assert aligned.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    pts, resp, cnt = eng.harris_keypoints(aligned, n)
    pts1, resp1, cnt1 = eng.harris_keypoints(shifted, n)
    for i in range(f):
        ep, er, ec = okp.key_points(noise_frames[i], n)
        assert ec == n                                       # the frames have more candidates than any n here
        assert int(cnt[i]) == ec and np.array_equal(pts[i].cpu().numpy(), ep) and np.array_equal(resp[i].cpu().numpy(), er)
        assert int(cnt1[i]) == ec and np.array_equal(pts1[i].cpu().numpy(), ep) and np.array_equal(resp1[i].cpu().numpy(), er)
    assert torch.equal(pts, pts1) and torch.equal(resp, resp1) and torch.equal(cnt, cnt1)


@pytest.mark.parametrize("h,w,tiles,n", [(33, 33, 4, 60), (64, 257, 18, 300)])
def test_harris_tile_counts(eng, h, w, tiles, n):
    """Frames of 2 x 2 and 2 x 9 tiles of 32 x 32 pixels, the last row / column of tiles one pixel deep or wide."""
    assert -(-h // 32) * -(-w // 32) == tiles
    img = np.random.RandomState(h * w).randint(0, 256, (1, h, w)).astype(np.uint8)
    pts, resp, cnt = eng.harris_keypoints(torch.from_numpy(img).to(eng.device), n)
    ep, er, ec = okp.key_points(img[0], n)
    assert int(cnt[0]) == ec and np.array_equal(pts[0].cpu().numpy(), ep) and np.array_equal(resp[0].cpu().numpy(), er)
