"""What the C entry points of the descriptor stage refuse, and the word they refuse it with: the plan word and the
64-row cap of SPLIT (dlc_pca_project, dlc_lsh_hash_i8), the workspace rule -- null, one byte short, a base 8 bytes off
16 -- (those two, dlc_vlad_encode, dlc_kmeans_step, dlc_verify_pairs, dlc_fuse_rows under SLAB) and an output that
shares a byte with an input (dlc_pca_project, dlc_lsh_quantize_i8, dlc_lsh_hash_i8, dlc_kmeans_step).  Status code and
dlc_last_error text are literals.  Every operand is carved out of one device arena, so "out on an input", "out on an
input's last element" and "out directly behind an input" are exact byte addresses; a call of the last kind is accepted
and writes the bits the same call writes into a buffer of its own.  A refused call launches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, BAD_SHAPE, WORKSPACE = 0, -1, -2, -5
F64 = 3
AUTO, ONE_PASS, SPLIT = 0, 1, 2

# byte offsets of the arena's regions (each on 256 bytes, each larger than what any case reads or writes of it)
X, BASIS, MEAN, SCALE, OUT, WS = 0x00000, 0x08000, 0x10000, 0x14000, 0x15000, 0x17000
Q8, PLANES, CODES = 0x20000, 0x28000, 0x30000
PTS, CAND, ASSIGN, PREV, SMALL = 0x31000, 0x32000, 0x33000, 0x34000, 0x35000
ARENA_BYTES = 0x36000


class Arena:
    def __init__(self, e):
        rng = np.random.RandomState(11)
        host = np.zeros(ARENA_BYTES, dtype=np.uint8)
        host[:Q8] = rng.uniform(-1.0, 1.0, Q8 // 8).view(np.uint8)                 # the fp64 regions
        host[Q8:CODES] = rng.randint(-127, 128, CODES - Q8).astype(np.int8).view(np.uint8)
        self.t = torch.from_numpy(host).to(e.device)
        self.base = self.t.data_ptr()
        assert self.base % 256 == 0

    def ptr(self, off):
        return C.c_void_p(self.base + off)

    def bytes(self, off, n):
        return self.t[off:off + n].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def e():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


@pytest.fixture(scope="module")
def A(e):
    return Arena(e)


def refused(e, rc, code, text):
    assert (rc, e.lib.dlc_last_error(e.ctx).decode()) == (code, text)


# the three workspaces a call that needs `need` bytes refuses: (pointer offset or None, bytes)
def bad_workspaces(need):
    return [(None, 0), (WS, need - 1), (WS + 8, need + 8)]


# ---- dlc_pca_project ----------------------------------------------------------------------------------------------------
def pca(e, A, rows=2, D=5, M=3, out=OUT, plan=ONE_PASS, ws=None, ws_bytes=0):
    return e.lib.dlc_pca_project(e.ctx, A.ptr(X), rows, D, D, A.ptr(MEAN), F64, A.ptr(BASIS), M, M, A.ptr(SCALE), A.ptr(out), M,
                                 plan, None if ws is None else A.ptr(ws), ws_bytes, e._stream())


def test_pca_plan(e, A):
    refused(e, pca(e, A, plan=3), BAD_ARG, "pca_project: unknown plan 3")
    refused(e, pca(e, A, rows=65, plan=SPLIT), BAD_SHAPE, "pca_project: DLC_PCA_PLAN_SPLIT takes at most 64 rows, not 65")


def test_pca_workspace(e, A):
    assert e.lib.dlc_pca_project_workspace_bytes(2, 1025, 3, SPLIT) == 256
    for ws, nbytes in bad_workspaces(256):
        refused(e, pca(e, A, D=1025, plan=SPLIT, ws=ws, ws_bytes=nbytes), WORKSPACE,
                "pca_project: needs 256 bytes of 16-byte aligned workspace")


def test_pca_overlap(e, A):
    for start, nbytes in ((X, 2 * 5 * 8), (MEAN, 5 * 8), (BASIS, 5 * 3 * 8), (SCALE, 3 * 8)):
        for out in (start, start + nbytes - 8):                       # on the input; on its last element alone
            refused(e, pca(e, A, out=out), BAD_ARG, "pca_project: out overlaps an input")
    assert pca(e, A) == OK
    assert pca(e, A, out=X + 2 * 5 * 8) == OK                         # directly behind x's last byte
    assert A.bytes(X + 2 * 5 * 8, 2 * 3 * 8) == A.bytes(OUT, 2 * 3 * 8)


# ---- dlc_lsh_quantize_i8, dlc_lsh_hash_i8 -------------------------------------------------------------------------------
def quantize(e, A, q):
    return e.lib.dlc_lsh_quantize_i8(e.ctx, F64, A.ptr(X), 2, 5, 5, A.ptr(MEAN), A.ptr(q), 5, e._stream())


def test_lsh_quantize_overlap(e, A):
    for start, nbytes in ((X, 2 * 5 * 8), (MEAN, 5 * 8)):
        for q in (start, start + nbytes - 1):                         # on the input; on its last byte alone
            refused(e, quantize(e, A, q), BAD_ARG, "lsh_quantize: q overlaps an input")
    assert quantize(e, A, CODES) == OK
    assert quantize(e, A, X + 2 * 5 * 8) == OK
    assert A.bytes(X + 2 * 5 * 8, 2 * 5) == A.bytes(CODES, 2 * 5)


def lsh_hash(e, A, rows=2, D=5, out=CODES, plan=ONE_PASS, ws=None, ws_bytes=0):
    ld = (D + 15) // 16 * 16
    return e.lib.dlc_lsh_hash_i8(e.ctx, A.ptr(Q8), rows, D, ld, A.ptr(PLANES), 3, ld, A.ptr(out), 16, plan,
                                 None if ws is None else A.ptr(ws), ws_bytes, e._stream())


def test_lsh_hash_plan(e, A):
    refused(e, lsh_hash(e, A, plan=3), BAD_ARG, "lsh_hash: unknown plan 3")
    refused(e, lsh_hash(e, A, rows=65, plan=SPLIT), BAD_SHAPE, "lsh_hash: DLC_LSH_PLAN_SPLIT takes at most 64 rows, not 65")


def test_lsh_hash_workspace(e, A):
    assert e.lib.dlc_lsh_hash_workspace_bytes(2, 8193, 3, SPLIT) == 2048
    for ws, nbytes in bad_workspaces(2048):
        refused(e, lsh_hash(e, A, D=8193, plan=SPLIT, ws=ws, ws_bytes=nbytes), WORKSPACE,
                "lsh_hash: needs 2048 bytes of 16-byte aligned workspace")


def test_lsh_hash_overlap(e, A):
    for start, nbytes in ((Q8, 16 + 5), (PLANES, 2 * 16 + 5)):
        for out in (start, start + nbytes - 1):
            refused(e, lsh_hash(e, A, out=out), BAD_ARG, "lsh_hash: out overlaps an input")
    assert lsh_hash(e, A) == OK
    assert lsh_hash(e, A, out=Q8 + 16 + 5) == OK                      # directly behind the last byte of q's last row
    assert A.bytes(Q8 + 16 + 5, 2 * 16) == A.bytes(CODES, 2 * 16)


# ---- dlc_vlad_encode, dlc_kmeans_step: rows of H = 4 against K = 2 words -------------------------------------------------
def test_vlad_encode_workspace(e, A):
    assert e.lib.dlc_vlad_encode_workspace_bytes(2, 2, 4, 2) == 256
    for ws, nbytes in bad_workspaces(256):
        rc = e.lib.dlc_vlad_encode(e.ctx, A.ptr(X), 2, 2, 4, 4, A.ptr(BASIS), 2, 4, 1, A.ptr(OUT), 8, None,
                                   None if ws is None else A.ptr(ws), nbytes, e._stream())
        refused(e, rc, WORKSPACE, "vlad_encode: needs 256 bytes of 16-byte aligned workspace")


def kmeans(e, A, c_out=OUT, out_assign=ASSIGN, small=SMALL, ws=WS, ws_bytes=256):
    return e.lib.dlc_kmeans_step(e.ctx, A.ptr(X), 2, 4, 4, A.ptr(BASIS), 2, 4, A.ptr(c_out), 4, A.ptr(PREV), A.ptr(out_assign),
                                 A.ptr(small), A.ptr(small + 16), A.ptr(small + 24), None if ws is None else A.ptr(ws), ws_bytes,
                                 e._stream())


def test_kmeans_step_workspace(e, A):
    assert e.lib.dlc_kmeans_step_workspace_bytes(2, 4, 2) == 256
    for ws, nbytes in bad_workspaces(256):
        refused(e, kmeans(e, A, ws=ws, ws_bytes=nbytes), WORKSPACE, "kmeans_step: needs 256 bytes of 16-byte aligned workspace")


def test_kmeans_step_overlap(e, A):
    for c_out in (BASIS, BASIS + 2 * 4 * 8 - 8):
        refused(e, kmeans(e, A, c_out=c_out), BAD_ARG, "kmeans_step: c_out overlaps c_in")
    for out_assign in (PREV, PREV + 2 * 4 - 4):
        refused(e, kmeans(e, A, out_assign=out_assign), BAD_ARG, "kmeans_step: out_assign overlaps prev_assign")
    assert kmeans(e, A) == OK
    # c_out directly behind c_in's last byte, out_assign directly behind prev_assign's
    assert kmeans(e, A, c_out=BASIS + 2 * 4 * 8, out_assign=PREV + 2 * 4, small=SMALL + 64) == OK
    assert A.bytes(BASIS + 2 * 4 * 8, 2 * 4 * 8) == A.bytes(OUT, 2 * 4 * 8)
    assert A.bytes(PREV + 2 * 4, 2 * 4) == A.bytes(ASSIGN, 2 * 4)
    assert A.bytes(SMALL + 64, 32) == A.bytes(SMALL, 32)              # counts [2], inertia, changed


# ---- dlc_verify_pairs, dlc_fuse_rows ------------------------------------------------------------------------------------
def test_verify_pairs_workspace(e, A):
    assert e.lib.dlc_verify_pairs_workspace_bytes(2, 1, 2) == 256
    for ws, nbytes in bad_workspaces(256):
        rc = e.lib.dlc_verify_pairs(e.ctx, A.ptr(X), 4, A.ptr(PTS), 2, A.ptr(BASIS), 4, A.ptr(PTS + 256), 2, 2, 4, A.ptr(CAND), 1, 1,
                                    0, 3, 32, 1, A.ptr(ASSIGN), A.ptr(ASSIGN + 256), None, None, None, None,
                                    None if ws is None else A.ptr(ws), nbytes, e._stream())
        refused(e, rc, WORKSPACE, "verify_pairs: needs 256 bytes of 16-byte aligned workspace")


def test_fuse_rows_slab_workspace(e, A):
    assert e.lib.dlc_fuse_rows_workspace_bytes(2, 5, 1) == 256
    for ws, nbytes in bad_workspaces(256):
        rc = e.lib.dlc_fuse_rows(e.ctx, 1, (C.c_int * 1)(F64), (C.c_void_p * 1)(A.base + X), (C.c_int64 * 1)(5),
                                 (C.c_double * 1)(1.0), (C.c_int * 1)(0), 2, 5, 5, 0, 1, 2, A.ptr(OUT), 5,
                                 None if ws is None else A.ptr(ws), nbytes, e._stream())
        refused(e, rc, WORKSPACE, "fuse_rows: needs 256 bytes of 16-byte aligned workspace")


# ---- the same plan rule in front of the library: Engine.pca_project, Engine.lsh_hash -------------------------------------
def test_engine_plan_refusals(e):
    def said(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    x = torch.zeros((65, 5), dtype=torch.float64, device=e.device)
    basis = torch.zeros((5, 3), dtype=torch.float64, device=e.device)
    assert said(lambda: e.pca_project(x[:2], basis, plan="bogus")) == \
        "pca_project: plan='bogus' is none of ['auto', 'one_pass', 'split']"
    assert said(lambda: e.pca_project(x, basis, plan="split")) == "pca_project: plan 'split' takes at most 64 rows, not 65"
    q = torch.zeros((65, 16), dtype=torch.int8, device=e.device)
    planes = torch.zeros((3, 16), dtype=torch.int8, device=e.device)
    assert said(lambda: e.lsh_hash(q[:2], planes, plan="bogus")) == "lsh_hash: plan='bogus' is none of ['auto', 'one_pass', 'split']"
    assert said(lambda: e.lsh_hash(q, planes, plan="split")) == "lsh_hash: plan 'split' takes at most 64 rows, not 65"
