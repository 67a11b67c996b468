"""The secure-aggregation rule (fedmi/parallel/secagg.py, csrc/kernels/secagg.hip) in plain numpy: the ChaCha20 block
function on uint32, and encode / mask / decode with fp64 where the rule says fp64.  Written apart from the package's
own numpy twin; the tests hold both, and the kernels, against this one bit for bit."""
import numpy as np

Q_MAX = 2 ** 27 - 1
M32 = 0xFFFFFFFF


def chacha20_block(key, counter, nonce) -> np.ndarray:
    """RFC 8439 section 2.3.  ``key``: 8 words, ``nonce``: 3 words, ``counter``: an array of block counters.  Returns
    ``[len(counter), 16]`` uint32, the output words in the RFC's order."""
    counter = np.atleast_1d(np.asarray(counter))
    st = np.zeros((16, counter.size), dtype=np.uint32)               # uint32 arrays wrap mod 2^32
    st[0], st[1], st[2], st[3] = 0x61707865, 0x3320646E, 0x79622D32, 0x6B206574
    for i in range(8):
        st[4 + i] = int(key[i]) & M32
    st[12] = (counter & M32).astype(np.uint32)
    for i in range(3):
        st[13 + i] = int(nonce[i]) & M32
    w = st.copy()

    def rot(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    def qr(a, b, c, d):
        w[a] += w[b]; w[d] = rot(w[d] ^ w[a], 16)
        w[c] += w[d]; w[b] = rot(w[b] ^ w[c], 12)
        w[a] += w[b]; w[d] = rot(w[d] ^ w[a], 8)
        w[c] += w[d]; w[b] = rot(w[b] ^ w[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return (w + st).T


def keystream(key, draw: int, n: int) -> np.ndarray:
    """``m[i]`` of one pair: block ``i >> 4`` under nonce ``(draw lo, draw hi, 0)``; within a block coordinate
    ``4 c + k`` takes output word ``4 k + c``."""
    nb = (n + 15) // 16
    blocks = np.ascontiguousarray(chacha20_block(key, np.arange(nb), (draw & M32, (draw >> 32) & M32, 0)))
    return blocks.reshape(nb, 4, 4).swapaxes(1, 2).reshape(-1)[:n]       # [B][k][c] -> [B][c][k], flat = 16 B + 4 c + k


def encode(x: np.ndarray, a: np.ndarray, f: int):
    """``(q int64, clamped)``: the fp32 difference, scaled exactly, clamped as a real number, rounded to even."""
    with np.errstate(all="ignore"):
        s = ((x.astype(np.float32) - a.astype(np.float32)) * np.float32(2.0 ** f)).astype(np.float64)
    nan = np.isnan(s)
    out = nan | (np.abs(s) > Q_MAX)
    q = np.rint(np.clip(np.where(nan, 0.0, s), -Q_MAX, Q_MAX)).astype(np.int64)
    return q, int(out.sum())


def mask(x, a, keys, rank: int, draw: int, f: int):
    """``(u uint32[n], clamped)`` of rank ``rank``; ``keys[j]`` = the 8 words shared with rank ``j``."""
    q, clamped = encode(x, a, f)
    u = q & M32
    for j in range(len(keys)):
        if j != rank:
            m = keystream(keys[j], draw, q.size).astype(np.int64)
            u = (u + m if j > rank else u - m) & M32
    return u.astype(np.uint32), clamped


def decode(rows: np.ndarray, a: np.ndarray, f: int) -> np.ndarray:
    """``a + (float)((double) S 2^-f / W)`` with ``S`` the rows' sum mod 2^32 read as int32."""
    total = rows.astype(np.int64).sum(0) & M32
    total = np.where(total >= 2 ** 31, total - 2 ** 32, total).astype(np.float64)
    m = (total * 2.0 ** -f / float(rows.shape[0])).astype(np.float32)
    return a.astype(np.float32) + m
