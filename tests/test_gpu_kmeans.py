"""csrc/avc_codebook.hip and avatarclip_amd/kmeans.py on the device against tests/kmeans_restatement.py.

Assignment criterion, against fp64: d1 <= d2 the two smallest fp64 distances of a point, tol = 64 * 2^-24 * (|x|^2 + |c|^2) with c the
nearest centre (64 * 2^-24 bounds the D + 2 fp32 roundings of one distance chain for D <= 32 relative to sum (x - c)^2 <= 2 (|x|^2 + |c|^2),
with room for either accumulation order).  Where d2 - d1 > tol the index must match exactly; elsewhere the chosen centre's fp64 distance is
<= d1 + tol; dist lies within tol of d1 everywhere.  tests/test_kmeans_cpu.py asserts, for these seeds, that at most 1 % of the points
lie inside the band.  kmeans.CENTRE_TILE is 0 (the kernel stages no tile of centres), so no case sits on a tile edge; the bit-identical
centres stand 59 apart and side by side in the kernel's ascending walk.

Update: counts exact, centres bit for bit the restatement's (ascending point index, sequential fp32, one division), within
2^-24 (sum |x_d| + |c_d|) of the fp64 mean, empty clusters untouched, two runs equal."""
import numpy as np
import pytest
import torch

from tests import kmeans_restatement as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assign(x, c):
    from avatarclip_amd import kmeans as KM
    a, d = KM.assign(torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV))
    torch.cuda.synchronize()
    return a.cpu().numpy(), d.cpu().numpy()


def _check_assignment(x, c, a, d):
    assert a.dtype == np.int32 and d.dtype == np.float32 and a.min() >= 0 and a.max() < len(c)
    d1, d2, i1, tol = R.band(x, c)
    dd = R.distances(x, c)
    chosen = dd[np.arange(len(x)), a]
    clear = d2 - d1 > tol
    print("points %d, in the band %d, max |dist - d1| / tol = %.3g" % (len(x), int((~clear).sum()), float((np.abs(d - d1) / np.maximum(tol, 1e-300)).max())))
    assert (a[clear] == i1[clear]).all()
    assert (chosen[~clear] <= d1[~clear] + tol[~clear]).all()
    assert (np.abs(d.astype(np.float64) - d1) <= tol).all()


@pytest.mark.parametrize("N,K,D", R.ASSIGN_CASES)
def test_assignment_against_fp64(N, K, D):
    x, c = R.assignment_inputs(N, K, D, R.case_seed(N, K, D))
    a, d = _assign(x, c)
    _check_assignment(x, c, a, d)


@pytest.mark.parametrize("D", [16, 32])
def test_bit_identical_centres_give_the_lower_index_and_an_equal_point_distance_zero(D):
    x, c, pts, owner, equal = R.tie_inputs(D)
    a, d = _assign(x, c)
    assert (a[pts] == owner).all() and 64 not in a and 21 not in a
    assert (d[equal] == 0).all() and a[130] == 40
    _check_assignment(x, c, a, d)
    again = _assign(x, c)
    assert (again[0] == a).all() and again[1].tobytes() == d.tobytes()


def test_the_library_refuses_other_widths_and_sizes():
    from avatarclip_amd import lib
    x, c = torch.zeros(8, 24, device=DEV), torch.zeros(2, 24, device=DEV)
    a, d = torch.empty(8, device=DEV, dtype=torch.int32), torch.empty(8, device=DEV)
    with pytest.raises(RuntimeError, match="D must be 16 or 32"):
        lib.call("avc_kmeans_assign", x, 8, 24, c, 2, a, d)
    with pytest.raises(RuntimeError, match="bad sizes"):
        lib.call("avc_kmeans_assign", x, 8, 16, c, 0, a, d)
    with pytest.raises(RuntimeError, match="D must be 16 or 32"):
        lib.call("avc_kmeans_update", torch.zeros(8, device=DEV, dtype=torch.int64), 8, x, 24, c, 2, a)


@pytest.mark.parametrize("D", [16, 32])
def test_update_is_the_restated_sum_bit_for_bit(D):
    from avatarclip_amd import kmeans as KM
    x, a, c = R.update_inputs(D)
    want, want_counts = R.update(x, a, c)
    xd, ad = torch.from_numpy(x).to(DEV), torch.from_numpy(a).to(DEV)
    runs = []
    for _ in range(2):
        cd = torch.from_numpy(c).to(DEV)
        counts = KM.update(xd, ad, cd)
        torch.cuda.synchronize()
        runs.append((cd.cpu().numpy(), counts.cpu().numpy()))
    got, counts = runs[0]
    assert counts.dtype == np.int32 and (counts == want_counts).all() and counts[13] == 0 and counts[14] == 1
    assert got.tobytes() == want.tobytes()
    assert got[13].tobytes() == c[13].tobytes()                                            # the empty cluster keeps its bits
    assert runs[1][0].tobytes() == got.tobytes() and (runs[1][1] == counts).all()
    x64 = x.astype(np.float64)
    for k in range(len(c)):
        if counts[k]:
            rows = x64[a == k]
            bound = 2.0 ** -24 * (np.abs(rows).sum(0) + np.abs(got[k]))
            assert (np.abs(got[k] - rows.mean(0)) <= bound).all(), k


def test_the_loop_on_five_blobs_reaches_the_restated_assignment():
    from avatarclip_amd import kmeans as KM
    x, init, label = R.blob_inputs()
    want_c, want_a, want = R.lloyd(x, init)
    xd = torch.from_numpy(x).to(DEV)
    c, a, info = KM.kmeans(xd, 5, init=torch.from_numpy(init).to(DEV))
    assert info["converged"] and info["changed"][-1] == 0 and info["changed"][0] == 1500 and info["empty"] == []
    assert (a.cpu().numpy() == want_a).all() and (want_a == label).all()
    assert info["iterations"] == want["iterations"] and info["changed"] == want["changed"]
    assert c.cpu().numpy().tobytes() == want_c.tobytes()                                   # equal assignments, the stated order: equal bits
    assert len(info["inertia"]) == info["iterations"] and info["inertia"][-1] == info["final_inertia"] <= info["inertia"][0]
    again, dist = KM.assign(xd, c)
    assert torch.equal(again, a)
    assert abs(float(dist.sum(dtype=torch.float64)) - info["final_inertia"]) <= 1e-9 * info["final_inertia"]
    c2, a2, info2 = KM.kmeans(xd, 5, init=torch.from_numpy(init).to(DEV))
    assert torch.equal(c2, c) and torch.equal(a2, a) and info2 == info


def test_seeded_initial_centres_and_the_iteration_limit():
    from avatarclip_amd import kmeans as KM
    x, _, _ = R.blob_inputs()
    xd = torch.from_numpy(x).to(DEV)
    perm = torch.randperm(1500, generator=torch.Generator().manual_seed(7))[:9]
    one = KM.kmeans(xd, 9, iters=2, seed=7)
    want_c, want_a, want = R.lloyd(x, x[perm.numpy()], iters=2)
    assert one[2]["iterations"] == 2 and one[2]["converged"] == want["converged"] and one[2]["changed"][0] == 1500
    two = KM.kmeans(xd, 9, iters=2, seed=7)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and one[2] == two[2]          # the same seed: the same bits
    assert torch.equal(KM.assign(xd, one[0])[0], one[1])                                             # also when the limit ended the loop
    assert torch.equal(KM.initial_centres(xd, 9, 7).cpu(), torch.from_numpy(x)[perm])
    if (one[1].cpu().numpy() == want_a).all():               # (a near-tie may differ from fp64 here; where it does not, the bits agree)
        assert one[0].cpu().numpy().tobytes() == want_c.tobytes()
