"""What the two batched-RANSAC mirrors (sim3_solver.py, pnp_solver.py) share on the Python side: the CSR batch (corr_off, hyp_off), the mask layout of
include/cubeslam_hip.h -- correspondence i is bit i & 31 of word i >> 5, ceil(N / 32) words per hypothesis --, and the reference's partial Fisher-Yates."""
import numpy as np


def f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1)


def i32(a):
    return np.ascontiguousarray(a, np.int32).reshape(-1)


def cat(parts, dt, w):
    """Rows of width w of every part, one under the other."""
    parts = list(parts)
    return np.concatenate([np.asarray(p, dt).reshape(-1, w) for p in parts]) if parts else np.zeros((0, w), dt)


def offsets(counts):
    """[0, c0, c0 + c1, ...] as int32."""
    return np.concatenate([[0], np.cumsum(list(counts))]).astype(np.int32)


def batch(corr_off, hyp_off):
    """-> corr_off, hyp_off as int32 arrays, n_problems, the number of correspondences, of hypotheses and of mask words."""
    co = np.ascontiguousarray(corr_off, np.int32); ho = np.ascontiguousarray(hyp_off, np.int32)
    n = len(co) - 1
    if len(ho) != n + 1:
        raise ValueError("corr_off and hyp_off must have one entry per problem and one more")
    NC, H = (int(co[-1]), int(ho[-1])) if n else (0, 0)
    return co, ho, n, NC, H, mask_words(co, ho)


def mask_words(co, ho):
    """The mask words of a batch; 0 for decreasing offsets (the library's to refuse)."""
    nh, N = np.diff(np.asarray(ho, np.int64)), np.diff(np.asarray(co, np.int64))
    return 0 if (nh < 0).any() or (N < 0).any() else int((nh * ((N + 31) // 32)).sum())


def mask_bits(words, N):
    """mvbInliersi of one hypothesis from its ceil(N / 32) mask words."""
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:N].astype(bool)


def problem_slices(flat, ho, Ns, masks=()):
    """The arrays of one call cut per problem: p -> {key: its hypotheses' rows, a copy}; the keys of `masks` are words, returned as (hypotheses, words of one)."""
    w0 = 0
    for p, N in enumerate(Ns):
        W, nh = (N + 31) // 32, int(ho[p + 1] - ho[p])
        yield {k: (v[w0:w0 + nh * W].reshape(nh, W) if k in masks else v[ho[p]:ho[p + 1]]).copy() for k, v in flat.items()}
        w0 += nh * W


def draw(N, k, count, random_int):
    """`count` sets of k distinct indices below N, (count, k) int32: the partial Fisher-Yates of the reference's iterate() over random_int(min, max), DUtils::Random::RandomInt."""
    out = np.zeros((count, k), np.int32)
    for it in range(count):
        vAvailableIndices = list(range(N))
        for i in range(k):
            randi = random_int(0, len(vAvailableIndices) - 1)
            out[it, i] = vAvailableIndices[randi]
            vAvailableIndices[randi] = vAvailableIndices[-1]
            vAvailableIndices.pop()
    return out
