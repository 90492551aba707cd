"""avatarclip_amd/lib.py derives the ctypes binding from include/avc.h: the parser on the real header and on strings, the marshalling
of L.call with a stub in place of the foreign function (no launch), and on the device four tiny launches through L.call against the
same launches through the raw idiom L.check(lib.avc_x(L.ptr(a), ..., L.stream()), "avc_x")."""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_void_p as P

import pytest
import torch

from avatarclip_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ = None       # a scalar parameter has no element type

# name -> (restype, argtypes, element types), written out from include/avc.h by hand
EXPECTED = {
    "avc_rig_cell_keys": (c_int, [P, c_int, c_double, c_double, c_double, c_double, c_int, P, P],
                          ["float", N_, N_, N_, N_, N_, N_, "long long", "void"]),
    "avc_rot_to_quat": (c_int, [P, c_long, P, P], ["float", N_, "float", "void"]),
    "avc_pack_params": (c_int, [P, c_int, P, P, c_int, P, P, c_int, P, P, P, P],
                        ["float", N_, "long", "float", N_, "long", "float", N_, "void", "void", "float", "void"]),
    "avc_mc_emit": (c_int, [P, c_int, c_int, c_int, c_float, P, P, P, P, P, P, P, P, P],
                    ["float", N_, N_, N_, N_, "int", "int", "int", "int", "signed char", "int", "float", "int", "void"]),
    "avc_preview_shade": (c_int, [P, P, c_int, c_int, P, c_int, P, c_int, P, c_float, c_float, c_float, c_float, c_float, c_int, c_int, P, P, P, P],
                          ["int", "float", N_, N_, "int", N_, "unsigned char", N_, "float", N_, N_, N_, N_, N_, N_, N_, "void", "unsigned char",
                           "int", "void"]),
    "avc_mesh_largest_island": (c_int, [P, c_int, c_int, P, P, P, P, P, P],
                                ["int", N_, N_, "int", "int", "unsigned long long", "int", "int", "void"]),
    "avc_weight_grad_all": (c_int, [P, c_int, P, c_int, c_int, P, c_long, P, P, c_int, c_int, c_int, P],
                            ["void", N_, "void", N_, N_, "int", N_, "float", "float", N_, N_, N_, "void"]),
    "avc_last_error": (c_char_p, [], []),
    "avc_colsum_scratch_bytes": (c_long, [], []),
}
QUERIES = {"avc_version", "avc_num_offsets", "avc_fwd_panel_tiles", "avc_grad_panel_tiles", "avc_mask_u16_per_block", "avc_bwd_colsum_floats",
           "avc_shade_loss_blocks"}
SIZES = {"avc_fwd_scratch_bytes_per_wave", "avc_bwd_colsum_rows", "avc_colsum_scratch_bytes", "avc_vit_workspace_bytes",
         "avc_rasterize_scratch_bytes", "avc_preview_scratch_bytes", "avc_smpl_grad_scratch_bytes"}


@pytest.fixture(scope="module")
def protos():
    with open(os.path.join(ROOT, "include", "avc.h")) as f:
        return L.parse_header(f.read())


def test_parser_on_the_real_header(protos):
    protos, abi = protos
    assert abi == 4 and len(protos) == 81
    for name, (res, args, elems) in EXPECTED.items():
        p = protos[name]
        assert p.restype is res and p.argtypes == args and [q.elem for q in p.params] == elems, name
    pk = protos["avc_pack_params"].params
    assert [q.name for q in pk] == ["flat", "nparam", "idx16", "scale16", "n16", "idx32", "scale32", "n32", "w_f16", "w_bf16", "tab", "stream"]
    assert [q.const for q in pk] == [True, False, True, True, False, True, True, False, False, False, False, False]
    assert pk[2].decl == "const long*" and pk[10].decl == "float*" and pk[1].decl == "int"
    # the two spellings no function above has
    assert protos["avc_mesh_compact"].params[1] == L.Param("colors", P, "const unsigned*", "unsigned", True)
    assert protos["avc_dense_params_fwd"].params[1] == L.Param("v", P, "const void* const*", "void*", True)
    covered = {e for name in EXPECTED for e in EXPECTED[name][2]} | {"unsigned", "void*"}
    assert {q.elem for p in protos.values() for q in p.params} == covered
    # launches and queries
    assert {n for n, p in protos.items() if not p.launch} == QUERIES | SIZES | {"avc_last_error"}
    for n in SIZES:
        assert protos[n].restype is c_long, n
    for n, p in protos.items():
        if p.launch:
            assert p.restype is c_int and p.params[-1] == L.Param("stream", P, "void*", "void", False), n


def test_parser_on_strings():
    text = """
    #define AVC_ABI_VERSION 7
    /* a comment with a prototype inside: int avc_not_this(int a); */
    int avc_spread(const float* x /* host */,   // the input
                   long   n,
                   /* out */ unsigned
                   long long * best,
                   void* stream);
    long avc_bytes(void);
    """
    protos, abi = L.parse_header(text)
    assert abi == 7 and sorted(protos) == ["avc_bytes", "avc_spread"]
    p = protos["avc_spread"]
    assert p.restype is c_int and p.argtypes == [P, c_long, P, P] and p.launch
    assert [(q.name, q.decl, q.elem, q.const) for q in p.params] == [
        ("x", "const float*", "float", True), ("n", "long", None, False), ("best", "unsigned long long*", "unsigned long long", False),
        ("stream", "void*", "void", False)]
    assert protos["avc_bytes"].restype is c_long and protos["avc_bytes"].params == () and not protos["avc_bytes"].launch
    for bad, words in (("int avc_f(const float* x, size_t n, void* stream);", ("avc_f", "`n`", "size_t")),
                       ("int avc_g(const half* x, void* stream);", ("avc_g", "`x`", "half")),
                       ("int avc_h(short n);", ("avc_h", "`n`", "short")),
                       ("int avc_i(int n, void (*done)(int), void* stream);", ("avc_i", "done")),
                       ("int avc_j(const float*, int n);", ("avc_j", "const float*", "no name")),
                       ("int avc_k(int);", ("avc_k", "no name")),
                       ("float avc_l(int n);", ("avc_l", "float"))):
        with pytest.raises(ValueError) as e:
            L.parse_header(bad)
        for w in words:
            assert w in str(e.value), (bad, str(e.value))


@pytest.fixture
def stub(monkeypatch, protos):
    """avc_inv_s bound to a Python function that records its arguments and returns stub.status"""
    L.load()

    def fn(*args):
        fn.calls.append(args)
        return fn.status
    fn.calls, fn.status = [], 0
    monkeypatch.setitem(L._launches, "avc_inv_s", L.bind(protos[0]["avc_inv_s"], fn))
    return fn


def test_call_marshals_without_a_launch(stub):
    with pytest.raises(TypeError) as e:
        L.call("avc_inv_s", torch.zeros(1, dtype=torch.float64), None, None, stream=0)
    for w in ("avc_inv_s", "`variance`", "const float*", "torch.float64"):
        assert w in str(e.value)
    with pytest.raises(ValueError) as e:
        L.call("avc_inv_s", None, None, torch.zeros(2, dtype=torch.float32), stream=0)
    for w in ("avc_inv_s", "`out`", "float*", "torch.float32", "cpu"):
        assert w in str(e.value)
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float16), torch.zeros(1, dtype=torch.bool)):
        with pytest.raises(TypeError):
            L.call("avc_inv_s", bad, None, None, stream=0)
    assert stub.calls == []
    arr = (ctypes.c_float * 2)(1.0, 2.0)
    vp = ctypes.c_void_p(64)
    L.call("avc_inv_s", None, 4096, arr, stream=77)
    L.call("avc_inv_s", vp, None, None, stream=0)
    (a, b, c, st), second = stub.calls
    assert a is None and b == 4096 and type(b) is int and c is arr and st == 77
    assert second[0] is vp and second[1:] == (None, None, 0)
    for args in ((None, None), (None, None, None, None)):
        with pytest.raises(TypeError, match=r"avc_inv_s\(\) (takes 3 positional arguments but 4 |missing 1 required positional)"):
            L.call("avc_inv_s", *args, stream=0)
    assert len(stub.calls) == 2
    stub.status = 1
    with pytest.raises(RuntimeError, match="^libavc avc_inv_s failed: "):
        L.call("avc_inv_s", None, None, None, stream=0)
    with pytest.raises(AttributeError, match="avc_version"):
        L.call("avc_version")


def test_dtype_rule_of_every_element_type(protos):
    """int / unsigned: 4 bytes, long / long long: 8, the chars: 1 (bool included), never a floating dtype; void: anything"""
    mk = lambda *elems: L.Proto("avc_t", c_int, tuple(L.Param("p%d" % i, P, e + "*", e, False) for i, e in enumerate(elems))
                                + (L.Param("stream", P, "void*", "void", False),))
    seen = []
    launch = L.bind(mk("int", "unsigned", "long", "long long", "unsigned long long", "signed char", "unsigned char", "void"),
                    lambda *a: seen.append(a) or 0)
    t = lambda dt: torch.zeros(1, dtype=dt)
    good = [torch.int32, torch.int32, torch.int64, torch.int64, torch.int64, torch.int8, torch.bool, torch.float64]
    for i in range(len(good)):
        for dt in (torch.float32, torch.float64, torch.float16, torch.int16, torch.int32, torch.int64, torch.uint8):
            args = [None] * len(good)
            args[i] = t(dt)
            if i == 7 or (not dt.is_floating_point and dt.itemsize == good[i].itemsize):
                with pytest.raises(ValueError):          # the dtype passes; a CPU tensor stops at the device check
                    launch(*args, stream=0)
            else:
                with pytest.raises(TypeError, match="`p%d`" % i):
                    launch(*args, stream=0)
    assert seen == []


@pytest.mark.gpu
def test_call_launches_what_the_raw_idiom_launches():
    dev, lib = "cuda", L.load()
    torch.manual_seed(5)
    f32 = dict(device=dev, dtype=torch.float32)

    def both(name, ins, out_shape, out_dtype):
        """one launch through L.call and one through the raw idiom, each into its own -1-filled output (the last argument of all four)"""
        outs = [torch.full(out_shape, -1, device=dev, dtype=out_dtype) for _ in range(2)]
        L.call(name, *ins, outs[0])
        L.check(getattr(lib, name)(*[L.ptr(a) if torch.is_tensor(a) else a for a in ins], L.ptr(outs[1]), L.stream()), name)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], torch.full_like(outs[0], -1)), name
        return outs[0]

    var = torch.full((1,), 0.3, **f32)
    inv = both("avc_inv_s", [var, None], (2,), torch.float32)
    assert abs(inv[0].item() * inv[1].item() - 1.0) < 1e-6
    M, J, T = 3, 2, 2
    joints = torch.randint(0, J, (M, 4), device=dev, dtype=torch.uint8)
    both("avc_skin_blend4", [joints, torch.rand(M, 4, **f32), torch.randn(T, J, 12, **f32), torch.randn(M, 3, **f32), M, J, T], (T, M, 3),
         torch.float32)
    rot = torch.linalg.qr(torch.randn(2, 3, 3, **f32))[0].contiguous()
    both("avc_rot_to_quat", [rot, 2], (2, 4), torch.float32)
    both("avc_rig_cell_keys", [torch.rand(4, 3, **f32), 4, 0.0, 0.0, 0.0, 0.25, 4], (4,), torch.int64)
    # a float64 tensor for `const float* variance` raises before anything is launched
    out, var64 = torch.full((2,), -1.0, **f32), var.double()
    torch.cuda.synchronize()
    with pytest.raises(TypeError, match="avc_inv_s.*`variance`.*const float\\*.*torch.float64"):
        L.call("avc_inv_s", var64, None, out)
    assert torch.cuda.current_stream().query()
    assert torch.equal(out, torch.full_like(out, -1.0))
