"""numpy restatement of avatarclip_amd/kmeans.py and csrc/avc_codebook.hip (the reference has no k-means to compare with: the oracle is this
file).  assign: fp64 distances in the direct form and the argmin, the lower index on a tie.  update: the kernel's stated summation order --
every cluster's points in ascending point index, sequentially, in fp32 from 0 -- then one fp32 division by the count; a cluster without
points keeps its centre.  lloyd: kmeans' loop on these two."""
import numpy as np


def distances(x, c):
    """[N,K] fp64 squared distances, sum over d of (x - c)^2"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(-1)


def assign(x, c):
    """(assign [N] int32, dist [N] fp64): np.argmin returns the first of equal minima, i.e. the lower index"""
    d = distances(x, c)
    a = np.argmin(d, axis=1)
    return a.astype(np.int32), d[np.arange(len(a)), a]


def update(x, a, c):
    """(centres [K,D] fp32, counts [K] int32) in the kernel's order and precision"""
    x, c = np.asarray(x, np.float32), np.array(c, np.float32, copy=True)
    counts = np.zeros(len(c), np.int32)
    for k in range(len(c)):
        idx = np.nonzero(np.asarray(a) == k)[0]            # ascending point index
        counts[k] = len(idx)
        if len(idx) == 0:
            continue
        s = np.zeros(x.shape[1], np.float32)
        for i in idx:
            s = (s + x[i]).astype(np.float32)
        c[k] = s / np.float32(len(idx))
    return c, counts


def lloyd(x, init, iters=100, assign_fn=assign):
    """kmeans.kmeans with given first centres -> (centres, assign, info with iterations / converged / changed / empty)"""
    c = np.array(init, np.float32, copy=True)
    prev = np.full(len(x), -1, np.int32)
    changed, counts, converged = [], None, False
    for _ in range(iters):
        a, _ = assign_fn(x, c)
        changed.append(int((a != prev).sum()))
        prev = a
        if changed[-1] == 0:
            converged = True
            break
        c, counts = update(x, a, c)
    if not converged:
        prev, _ = assign_fn(x, c)
    empty = [] if counts is None else [int(k) for k in np.nonzero(counts == 0)[0]]
    return c, prev, {"iterations": len(changed), "converged": converged, "changed": changed, "empty": empty}


# ---- what the GPU test's criterion needs, shared with the CPU test that checks the condition on its inputs
def band(x, c):
    """per point: (d1, d2 the two smallest fp64 distances (d2 = inf for K = 1), index of d1, tol = 64 * 2^-24 * (|x|^2 + |c|^2) with c the
    nearest centre)"""
    d = distances(x, c)
    order = np.argsort(d, axis=1, kind="stable")
    i1 = order[:, 0]
    d1 = d[np.arange(len(d)), i1]
    d2 = d[np.arange(len(d)), order[:, 1]] if d.shape[1] > 1 else np.full(len(d), np.inf)
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    tol = 64.0 * 2.0 ** -24 * ((x64 ** 2).sum(-1) + (c64[i1] ** 2).sum(-1))
    return d1, d2, i1, tol


def assignment_inputs(N, K, D, seed):
    """the GPU test's points and centres: standard-normal points, the centres drawn from them without replacement"""
    r = np.random.RandomState(seed)
    x = r.randn(N, D).astype(np.float32)
    pool = x if N >= K else r.randn(K, D).astype(np.float32)
    c = pool[r.permutation(len(pool))[:K]].copy()
    return x, c


ASSIGN_CASES = [(N, K, D) for D in (16, 32) for N in (1, 63, 1031) for K in (1, 67, 130)]
ASSIGN_SEED = 20


def case_seed(N, K, D):
    return ASSIGN_SEED + 1000 * D + 7 * N + K


def tie_inputs(D, seed=5):
    """K = 67 centres of which 5 / 64 and 20 / 21 are bit-identical pairs (far apart in the walk, and neighbours in it); 256 points: 64
    around each pair, 2 equal to the pairs' centres, the rest elsewhere.  -> (x, c, the points that belong to a pair, the lower index of
    their pair, the points equal to a centre)"""
    r = np.random.RandomState(seed + D)
    c = r.randn(67, D).astype(np.float32)
    c[64], c[21] = c[5], c[20]
    x = r.randn(256, D).astype(np.float32)
    x[:64] = c[5] + 0.01 * r.randn(64, D).astype(np.float32)
    x[64:128] = c[20] + 0.01 * r.randn(64, D).astype(np.float32)
    x[128], x[129] = c[5], c[20]
    x[130] = c[40]
    owner = np.concatenate([np.full(64, 5), np.full(64, 20), [5, 20]]).astype(np.int32)
    return x, c, np.arange(130), owner, np.array([128, 129, 130])


def blob_inputs(seed=3):
    """five well-separated blobs (centres 12 apart per coordinate pattern, spread 1) of 300 points each, N = 1500, D = 16, shuffled; init =
    one point per blob"""
    r = np.random.RandomState(seed)
    means = 6.0 * r.choice([-1.0, 1.0], size=(5, 16))
    while len({tuple(m) for m in means}) < 5:
        means = 6.0 * r.choice([-1.0, 1.0], size=(5, 16))
    label = r.permutation(np.repeat(np.arange(5), 300))
    x = (means[label] + r.randn(1500, 16)).astype(np.float32)
    init = np.stack([x[np.nonzero(label == b)[0][0]] for b in range(5)])
    return x, init, label


def update_inputs(D, seed=9):
    """1031 points in K = 67 clusters: cluster 13 has no point, cluster 14 exactly one, the sizes are otherwise random"""
    r = np.random.RandomState(seed + D)
    x = (r.randn(1031, D) * 3.0 + 1.0).astype(np.float32)
    a = r.randint(0, 67, size=1031).astype(np.int32)
    a[a == 13] = 12
    a[a == 14] = 15
    a[500] = 14
    c = r.randn(67, D).astype(np.float32)
    return x, a, c
