"""k-means without a GPU: the numpy restatement against brute force, the refusals of kmeans.kmeans before any launch, the third header of
the C ABI, and the condition the GPU test's criterion puts on its inputs (tests/test_gpu_kmeans.py)."""
import os

import numpy as np
import pytest
import torch

from tests import kmeans_restatement as R


def test_the_restated_assignment_is_brute_force_with_the_lower_index_on_ties():
    r = np.random.RandomState(0)
    x, c = r.randn(40, 16).astype(np.float32), r.randn(9, 16).astype(np.float32)
    c[7] = c[2]                                                # a tie for every point near them
    x[:5] = c[2] + 0.01 * r.randn(5, 16).astype(np.float32)
    a, d = R.assign(x, c)
    for i in range(len(x)):
        best, bd = 0, None
        for k in range(len(c)):
            dk = sum((float(x[i, j]) - float(c[k, j])) ** 2 for j in range(16))
            if bd is None or dk < bd:
                best, bd = k, dk
        assert a[i] == best and abs(d[i] - bd) <= 1e-12 * max(bd, 1.0), i
    assert set(a[:5]) == {2} and 7 not in a


def test_the_restated_update_sums_in_ascending_point_index_in_fp32_and_leaves_empty_clusters():
    x, a, c = R.update_inputs(16)
    new, counts = R.update(x, a, c)
    assert counts.dtype == np.int32 and counts.sum() == len(x) and counts[13] == 0 and counts[14] == 1
    assert new[13].tobytes() == c[13].tobytes() and new[14].tobytes() == x[500].tobytes()
    k = 3
    s = np.float32(0)
    for i in range(len(x)):                                    # by hand, one coordinate of one cluster
        if a[i] == k:
            s = np.float32(s + x[i, 5])
    assert new[k, 5] == np.float32(s / np.float32(counts[k]))
    mean64 = np.stack([x[a == j].astype(np.float64).mean(0) if (a == j).any() else c[j].astype(np.float64) for j in range(67)])
    bound = 2.0 ** -24 * (np.stack([np.abs(x[a == j].astype(np.float64)).sum(0) for j in range(67)]) + np.abs(new))
    assert (np.abs(new - mean64) <= bound).all()               # the bound the GPU test applies to the kernel holds for the stated order


def test_the_restated_loop_finds_five_blobs_and_stops_when_nothing_changes():
    x, init, label = R.blob_inputs()
    c, a, info = R.lloyd(x, init)
    assert info["converged"] and info["changed"][-1] == 0 and info["changed"][0] == len(x) and info["empty"] == []
    assert (a == label).all() and info["iterations"] <= 4      # init[b] is a point of blob b: cluster b IS blob b
    again, _ = R.assign(x, c)
    assert (again == a).all()
    two = R.lloyd(x, init, iters=1)                            # the limit: assigned once more to the updated centres
    assert not two[2]["converged"] and two[2]["iterations"] == 1 and (R.assign(x, two[0])[0] == two[1]).all()


def test_kmeans_refuses_before_any_launch(monkeypatch):
    from avatarclip_amd import kmeans as KM, lib
    monkeypatch.setattr(lib, "call", lambda *a, **k: pytest.fail("a refused call reached the library"))
    x = torch.randn(10, 16)
    with pytest.raises(ValueError, match="k = 11 centres but only 10 points"):
        KM.kmeans(x, 11)
    with pytest.raises(ValueError, match="at least 1"):
        KM.kmeans(x, 0)
    with pytest.raises(ValueError, match="D = 16 or 32"):
        KM.kmeans(torch.randn(10, 24), 2)
    with pytest.raises(ValueError, match=r"\[rows, D\]"):
        KM.kmeans(torch.randn(10), 2)
    bad = x.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="x holds a value that is not finite"):
        KM.kmeans(bad, 2)
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        KM.kmeans(bad, 2)
    with pytest.raises(ValueError, match="init holds a value that is not finite"):
        KM.kmeans(x, 2, init=torch.full((2, 16), float("inf")))
    with pytest.raises(ValueError, match=r"init must be \[k, D\]"):
        KM.kmeans(x, 2, init=torch.zeros(3, 16))
    with pytest.raises(ValueError, match="iters"):
        KM.kmeans(x, 2, iters=0)
    huge = torch.zeros(1, 16).expand(2 ** 27, 16)             # N D = 2^31 without the memory: refused by its shape alone
    with pytest.raises(ValueError, match="reaches 2\\^31"):
        KM.kmeans(huge, 2)
    with pytest.raises(ValueError, match="exceeds 65536"):
        KM.kmeans(torch.zeros(1, 16).expand(70000, 16), 65537)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # a valid host tensor: an error, not a quiet host path
        KM.kmeans(x, 2)
    assert KM.CENTRE_TILE == 0 and KM.DIMS == (16, 32)


def test_the_codebook_header_parses_and_the_other_two_keep_their_counts():
    """the k-means entry points live in a third header beside their source: it parses, every entry is a launch ending in `void* stream`,
    include/avc.h keeps its 81 prototypes and csrc/avc_texture.h its 2, no name is declared twice, and the binding merges the three"""
    from avatarclip_amd import build, lib
    protos, abi = lib.parse_header(open(lib.CODEBOOK_HEADER).read())
    assert abi is None and sorted(protos) == ["avc_kmeans_assign", "avc_kmeans_update"]
    for name, p in protos.items():
        assert p.launch and p.restype is lib.c_int and p.params[-1] == lib.Param("stream", lib.c_void_p, "void*", "void", False), name
    assert [q.name for q in protos["avc_kmeans_assign"].params] == ["x", "N", "D", "c", "K", "assign", "dist", "stream"]
    assert [(q.elem, q.const) for q in protos["avc_kmeans_assign"].params if q.elem] == [("float", True), ("float", True), ("int", False),
                                                                                        ("float", False), ("void", False)]
    assert protos["avc_kmeans_update"].params[0].elem == "long long" and protos["avc_kmeans_update"].params[-2].elem == "int"
    grey, abi_grey = lib.parse_header(open(lib.HEADER).read())
    tex, _ = lib.parse_header(open(lib.TEXTURE_HEADER).read())
    assert len(grey) == 81 and len(tex) == 2 and abi_grey == 4
    assert not set(grey) & set(tex) and not set(grey) & set(protos) and not set(tex) & set(protos)
    assert lib.headers() == (lib.HEADER, lib.TEXTURE_HEADER, lib.CODEBOOK_HEADER)
    assert os.path.samefile(lib.CODEBOOK_HEADER, os.path.join(build.CSRC, build.CODEBOOK_HEADER))
    assert build.CODEBOOK_HEADER in build.HEADERS and "avc_codebook.hip" in build.SOURCES
    bound = lib.load()
    assert lib.ABI_VERSION == 4 and bound.avc_version() == 4
    for name in protos:
        assert name in lib._launches and len(getattr(bound, name).argtypes) == len(protos[name].params)
    with pytest.raises(AttributeError, match=r"include/avc\.h, csrc/avc_texture\.h and csrc/avc_codebook\.h declare no launch entry point avc_nothing"):
        lib.call("avc_nothing")


def test_a_name_declared_in_two_headers_is_refused(tmp_path, monkeypatch):
    from avatarclip_amd import lib
    dup = tmp_path / "dup.h"
    dup.write_text("int avc_rasterize_mesh_tex_grad(const float* x, int N, void* stream);\n")
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "CODEBOOK_HEADER", str(dup))
    with pytest.raises(RuntimeError, match="declares avc_rasterize_mesh_tex_grad, which .*avc_texture.h declares already"):
        lib.load()


@pytest.mark.parametrize("N,K,D", [c for c in R.ASSIGN_CASES if c[1] > 1])
def test_the_assignment_inputs_keep_out_of_the_ambiguity_band(N, K, D):
    """the GPU test compares indices exactly only where d2 - d1 > tol = 64 * 2^-24 * (|x|^2 + |c|^2); its inputs must put at most 1 % of the
    points inside that band (a condition on the inputs, asserted here for the exact seeds it uses)"""
    x, c = R.assignment_inputs(N, K, D, R.case_seed(N, K, D))
    d1, d2, _, tol = R.band(x, c)
    inside = int((d2 - d1 <= tol).sum())
    assert inside <= 0.01 * N, (inside, N)


def test_the_band_is_nearly_empty_for_this_kind_of_input():
    """standard-normal points with centres drawn from them: fp64 puts a handful of 4099 points at most inside the band (relative width
    ~4e-6 of distances ~30) at (K, D) = (67, 16), (67, 32), (130, 32) -- the kind of input the per-case condition above is asserted on"""
    for K, D in ((67, 16), (67, 32), (130, 32)):
        x, c = R.assignment_inputs(4099, K, D, 1)
        d1, d2, _, tol = R.band(x, c)
        assert int((d2 - d1 <= tol).sum()) <= 4, (K, D)


@pytest.mark.parametrize("D", [16, 32])
def test_the_tie_inputs_hold_exact_ties_only_where_they_are_planted(D):
    x, c, pts, owner, equal = R.tie_inputs(D)
    assert c[5].tobytes() == c[64].tobytes() and c[20].tobytes() == c[21].tobytes()
    a, d = R.assign(x, c)
    assert (a[pts] == owner).all() and (d[equal] == 0).all()
    dd = R.distances(x[pts], c)
    assert (dd[np.arange(len(pts)), owner] == dd[np.arange(len(pts)), np.where(owner == 5, 64, 21)]).all()
    rest = np.setdiff1d(np.arange(len(x)), pts)
    d1, d2, i1, tol = R.band(x[rest], c)
    assert (d2 - d1 > tol)[~np.isin(i1, (5, 20))].all()        # a free point is in a tie only when a planted pair is its nearest
