"""Lloyd's k-means on the device: what makes the centres of the shape and pose CLIP codebooks (codebook.py).  The reference ships those
codebooks and no code that builds them (AvatarGen/ShapeGen/main.py:86-91, AvatarAnimate/models/pose_generation.py:298-300 only load them);
the paper clusters latents of the shape VAE and VPoser latents of a pose corpus by K-Means.

Two launches per iteration (csrc/avc_codebook.hip, declared in csrc/avc_codebook.h):

  assign   avc_kmeans_assign: per point the nearest centre by the direct squared distance sum (x - c)^2, the LOWER index on a tie
  update   the host sorts the words (assign << 32) | index -- the pattern of rig.simplify_mesh's cells -- and avc_kmeans_update sums every
           run sequentially in ascending point index in fp32 and divides by the count.  A cluster without points keeps its centre bit for
           bit.  No atomics: the same input gives the same bits in every run.

The only value the host reads per iteration is the number of points whose assignment changed; inertia and the empty clusters stay on the
device until the loop ends.  tests/kmeans_restatement.py restates both launches and the loop in numpy."""
import torch

from . import lib as L

DIMS = (16, 32)          # the widths avc_kmeans_assign is compiled for: ShapeGen's LinearVAE codes and VPoser's latents
MAX_K = 65536
CENTRE_TILE = 0          # avc_kmeans_assign stages no tile of centres: every centre reaches the lanes as scalar operands, in ascending index


def check_sizes(N, D, K):
    """the refusals that need no data, before any launch"""
    if D not in DIMS:
        raise ValueError("kmeans: points have D = 16 or 32 coordinates (the shape and pose latents), got D = %d" % D)
    if N < 1:
        raise ValueError("kmeans: no points")
    if N * D >= 2 ** 31:
        raise ValueError("kmeans: N D = %d x %d reaches 2^31; cluster a sample of the points" % (N, D))
    if K < 1:
        raise ValueError("kmeans: k must be at least 1, got %d" % K)
    if K > N:
        raise ValueError("kmeans: k = %d centres but only %d points" % (K, N))
    if K > MAX_K:
        raise ValueError("kmeans: k = %d exceeds %d" % (K, MAX_K))


def _matrix(t, what):
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError("kmeans: %s must be a [rows, D] tensor, got %s" % (what, list(t.shape) if torch.is_tensor(t) else type(t).__name__))
    return t


def assign(x, centres):
    """avc_kmeans_assign on device tensors x [N,D], centres [K,D] fp32 -> (assign [N] int32, dist [N] fp32)"""
    N, D, K = x.shape[0], x.shape[1], centres.shape[0]
    a = torch.empty(N, device=x.device, dtype=torch.int32)
    d = torch.empty(N, device=x.device, dtype=torch.float32)
    L.call("avc_kmeans_assign", x, N, D, centres, K, a, d)
    return a, d


def update(x, assignment, centres):
    """avc_kmeans_update: `centres` [K,D] is rewritten IN PLACE with the means of `assignment`'s clusters (empty ones untouched) -> counts
    [K] int32"""
    N, D, K = x.shape[0], x.shape[1], centres.shape[0]
    keys = (assignment.to(torch.int64) << 32) | torch.arange(N, device=x.device, dtype=torch.int64)
    keys = torch.sort(keys).values                         # distinct words: a cluster is a run, its points ascending
    counts = torch.empty(K, device=x.device, dtype=torch.int32)
    L.call("avc_kmeans_update", keys, N, x, D, centres, K, counts)
    return counts


def initial_centres(x, k, seed):
    """the k rows x[torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:k]] (the permutation is drawn on the host)"""
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(int(seed)))[:k]
    return x[perm.to(x.device)].clone()


def kmeans(x, k, iters=100, seed=0, init=None):
    """Lloyd's algorithm.  x [N,D] fp32 (D = 16 or 32), k centres; `init` [k,D] gives the first centres, None draws them with
    initial_centres(x, k, seed).  An iteration assigns every point and, when an assignment changed, recomputes the centres; the loop stops
    after the iteration in which none changed (the returned centres are then the ones the returned assignment was made with) or after
    `iters` iterations (the points are then assigned once more to the last centres, so the same holds).

    -> (centres [k,D] fp32, assign [N] int32, info): info["iterations"], info["converged"], info["changed"] (per iteration),
    info["inertia"] (per iteration: the fp64 sum of the squared distances of that iteration's assignment), info["final_inertia"] (of the
    returned assignment), info["empty"] (the clusters that had no point in the last update and kept their centre; sorted)."""
    x = _matrix(x, "x")
    N, D, k, iters = int(x.shape[0]), int(x.shape[1]), int(k), int(iters)
    check_sizes(N, D, k)
    if iters < 1:
        raise ValueError("kmeans: iters must be at least 1, got %d" % iters)
    if init is not None:
        init = _matrix(init, "init")
        if tuple(init.shape) != (k, D):
            raise ValueError("kmeans: init must be [k, D] = [%d, %d], got %s" % (k, D, list(init.shape)))
    for t, what in ((x, "x"), (init, "init")):
        if t is not None and not bool(torch.isfinite(t).all()):
            raise ValueError("kmeans: %s holds a value that is not finite" % what)
    if not x.is_cuda:
        raise RuntimeError("kmeans runs on the HIP kernels of libavc.so: x must be a device tensor; there is no CPU fallback")
    x = x.to(torch.float32).contiguous()
    centres = initial_centres(x, k, seed) if init is None else init.to(device=x.device, dtype=torch.float32).contiguous().clone()
    prev = torch.full((N,), -1, device=x.device, dtype=torch.int32)
    changed, inertia, counts, converged = [], [], None, False
    for _ in range(iters):
        a, d = assign(x, centres)
        inertia.append(d.sum(dtype=torch.float64))
        n = int((a != prev).sum().item())                  # the one host read of the iteration
        changed.append(n)
        prev = a
        if n == 0:
            converged = True
            break
        counts = update(x, a, centres)
    if not converged:
        prev, d = assign(x, centres)
        final = d.sum(dtype=torch.float64)
    else:
        final = inertia[-1]
    info = {"iterations": len(changed), "converged": converged, "changed": changed,
            "inertia": [float(v) for v in torch.stack(inertia).cpu()], "final_inertia": float(final),
            "empty": [] if counts is None else [int(i) for i in torch.nonzero(counts == 0).reshape(-1).cpu()]}
    return centres, prev, info
