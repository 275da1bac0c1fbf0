"""NumPy restatement of the two LDB definitions of include/dlc.h: dlc_ldb_describe_u8 (the thumbnail by
seqslam_oracle.resize, then per level the quadrant sums of every cell as slices, the pairs as two nested loops' index
lists, the bits packed least significant first) and dlc_hamming_rows (a 256-entry bit-count table over the xor).
Written from the header's text, not from the kernels: no lane groups, no decoded bit indices."""
import numpy as np

from seqslam_oracle import offered, resize  # noqa: F401  (offered: for the tests of the limits)


def valid_levels(levels):
    levels = list(levels)
    return 1 <= len(levels) <= 4 and all(isinstance(g, (int, np.integer)) and 2 <= g <= 8 for g in levels) and \
        all(a < b for a, b in zip(levels, levels[1:]))


def n_bits(levels):
    """3 * sum g^2 (g^2 - 1) / 2."""
    assert valid_levels(levels)
    return 3 * sum(g * g * (g * g - 1) // 2 for g in levels)


def row_bytes(levels):
    """16 * ceil(bits / 128)."""
    return 16 * ((n_bits(levels) + 127) // 128)


def cell_values(thumb, g):
    """thumb int64 [h, w] -> (S, DX, DY), each int64 [g * g], cell c = cy * g + cx."""
    h, w = thumb.shape
    assert h % (2 * g) == 0 and w % (2 * g) == 0
    ch, cw = h // g, w // g
    s, dx, dy = [], [], []
    for cy in range(g):
        for cx in range(g):
            c = thumb[cy * ch:(cy + 1) * ch, cx * cw:(cx + 1) * cw]
            q00, q01 = int(c[:ch // 2, :cw // 2].sum()), int(c[:ch // 2, cw // 2:].sum())
            q10, q11 = int(c[ch // 2:, :cw // 2].sum()), int(c[ch // 2:, cw // 2:].sum())
            s.append(q00 + q01 + q10 + q11)
            dx.append((q01 + q11) - (q00 + q10))
            dy.append((q10 + q11) - (q00 + q01))
    return np.array(s, np.int64), np.array(dx, np.int64), np.array(dy, np.int64)


def bits_of(thumb, levels):
    """thumb int64 [h, w] -> uint8 [n_bits] of 0 / 1, in the header's order."""
    out = []
    for g in levels:
        s, dx, dy = cell_values(thumb, g)
        n = g * g
        a = np.array([i for i in range(n) for j in range(i + 1, n)], dtype=np.int64)
        b = np.array([j for i in range(n) for j in range(i + 1, n)], dtype=np.int64)
        out.append(np.stack([s[a] > s[b], dx[a] > dx[b], dy[a] > dy[b]], axis=1).reshape(-1))
    return np.concatenate(out).astype(np.uint8)


def pack(bits, nbytes):
    """Bit t -> bit t & 7 of byte t >> 3; the rest of the nbytes bytes 0."""
    full = np.zeros(8 * nbytes, np.uint8)
    full[:len(bits)] = bits
    return np.packbits(full, bitorder="little")


def describe_thumbs(thumbs, levels):
    """thumbs integer [F, h, w] -> uint8 [F, row_bytes]: the rows of thumbnails that are already resized."""
    nb = row_bytes(levels)
    thumbs = np.asarray(thumbs).astype(np.int64)
    return np.stack([pack(bits_of(t, levels), nb) for t in thumbs]) if len(thumbs) else np.empty((0, nb), np.uint8)


def describe(gray, size, levels):
    """gray uint8 [F, H, W] -> uint8 [F, row_bytes]."""
    gray = np.asarray(gray)
    assert gray.dtype == np.uint8 and gray.ndim == 3
    return describe_thumbs(resize(gray, size[0], size[1]), levels)


POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


def hamming_rows(q, db):
    """int64 [Q, N]: sum_p popcount(q_r[p] ^ db_j[p]) on bytes."""
    q, db = np.asarray(q), np.asarray(db)
    assert q.dtype == np.uint8 and db.dtype == np.uint8
    out = np.empty((q.shape[0], db.shape[0]), dtype=np.int64)
    for r in range(q.shape[0]):
        out[r] = POPCOUNT[q[r][None, :] ^ db].sum(axis=1)
    return out
