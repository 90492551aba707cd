"""ctypes binding of libavc.so.  include/avc.h declares the C ABI, csrc/avc_texture.h the textured-render entry points and
csrc/avc_codebook.h the k-means entry points added beside it, csrc/avc_preview_clip.h the preview's clipping entry points: load() parses the
tuple headers() returns, then added_headers(), then later_headers() (csrc/avc_bake.h: the texture bake and the preview's textured shade), merges their prototypes and derives every restype / argtypes from them, and call() checks each tensor against the element type the header gives its parameter.  No
fallback: if the library is missing, lacks a symbol the header declares, or a call fails, an exception is raised."""
import collections
import ctypes
import os
import re

import torch

from . import build as _build

_lib = None
_launches = {}           # name -> the launcher bind() made, one per launch entry point (filled by load())
ABI_VERSION = None       # AVC_ABI_VERSION of include/avc.h (set by load())
HEADER = os.path.normpath(os.path.join(_build.CSRC, _build.ABI_HEADER))
TEXTURE_HEADER = os.path.join(_build.CSRC, _build.TEXTURE_HEADER)     # more entry points of the same library and revision (it defines no AVC_ABI_VERSION)
CODEBOOK_HEADER = os.path.join(_build.CSRC, _build.CODEBOOK_HEADER)   # the k-means entry points, likewise


PREVIEW_CLIP_HEADER = os.path.join(_build.CSRC, _build.PREVIEW_CLIP_HEADER)   # the preview's clipping entry points, likewise
BAKE_HEADER = os.path.join(_build.CSRC, _build.BAKE_HEADER)                   # the texture bake's entry points and the textured shade, likewise


def headers():
    """the tuple of headers load() parses, in this order (read when called); a name that two of them declare is refused"""
    return (HEADER, TEXTURE_HEADER, CODEBOOK_HEADER)


def added_headers():
    """the headers load() parses after headers(), under the same rules (read when called): entry points declared beside their source
    since the three above were fixed"""
    return (PREVIEW_CLIP_HEADER,)


def later_headers():
    """the headers load() parses last, after added_headers() and under the same rules (read when called)"""
    return (BAKE_HEADER,)


c_int, c_long, c_float, c_double, c_void_p, c_char_p = (ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_double,
                                                        ctypes.c_void_p, ctypes.c_char_p)

_SCALARS = {"int": c_int, "long": c_long, "float": c_float, "double": c_double}
_RETURNS = {"int": c_int, "long": c_long, "const char*": c_char_p}
_INTS = [getattr(torch, n) for n in ("bool", "int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64") if hasattr(torch, n)]
_FLOAT32, _FLOAT64 = frozenset([torch.float32]), frozenset([torch.float64])
_INT1, _INT4, _INT8 = (frozenset(d for d in _INTS if d.itemsize == n) for n in (1, 4, 8))
# element type of a pointer parameter -> the tensor dtypes it takes (None: any).  "void*" is the element of the host arrays of pointers.
_ELEMENTS = {"float": _FLOAT32, "double": _FLOAT64, "int": _INT4, "unsigned": _INT4, "long": _INT8, "long long": _INT8, "unsigned long long": _INT8,
             "void*": _INT8, "signed char": _INT1, "unsigned char": _INT1, "void": None}
_TYPE_WORDS = {"const", "void", "char", "short", "int", "long", "float", "double", "signed", "unsigned"}

# a parameter: its name, ctypes type and C type as declared; for a pointer also the element type and whether that is const
Param = collections.namedtuple("Param", "name ctype decl elem const")


class Proto(collections.namedtuple("Proto", "name restype params")):
    @property
    def argtypes(self):
        return [p.ctype for p in self.params]

    @property
    def launch(self):
        """a launch returns a status and ends in `void* stream`; everything else is a query"""
        return self.restype is c_int and bool(self.params) and self.params[-1][:3:2] == ("stream", "void*")


def _spell(tokens):
    return " ".join(tokens).replace(" *", "*")


def parse_header(text):
    """(the prototypes of a C header in the style of include/avc.h as {name: Proto}, its AVC_ABI_VERSION or None).  A declaration
    this cannot map raises ValueError."""
    abi = re.search(r"^\s*#\s*define\s+AVC_ABI_VERSION\s+(\d+)\s*$", text, flags=re.M)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    protos = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if not m:
            raise ValueError("cannot parse the declaration %r" % stmt)
        name = m.group(2)
        ret = _spell(m.group(1).replace("*", " * ").split())
        if ret not in _RETURNS:
            raise ValueError("%s: unknown return type `%s`" % (name, ret))
        params = []
        plist = m.group(3).strip()
        for i, p in enumerate([] if plist in ("", "void") else plist.split(",")):
            if "(" in p or ")" in p or "[" in p:
                raise ValueError("%s: parameter %d `%s` is a function pointer or an array" % (name, i + 1, p.strip()))
            tok = p.replace("*", " * ").split()
            if len(tok) < 2 or tok[-1] == "*" or tok[-1] in _TYPE_WORDS or not re.fullmatch(r"[A-Za-z_]\w*", tok[-1]):
                raise ValueError("%s: parameter %d `%s` has no name" % (name, i + 1, p.strip()))
            pname, tok = tok[-1], tok[:-1]
            decl = _spell(tok)
            if "*" in tok:
                pointee = tok[:len(tok) - 1 - tok[::-1].index("*")]
                elem = _spell([t for t in pointee if t != "const"])
                if elem not in _ELEMENTS:
                    raise ValueError("%s: parameter `%s` points to the unknown type `%s`" % (name, pname, elem))
                params.append(Param(pname, c_void_p, decl, elem, "const" in pointee))
            elif decl in _SCALARS:
                params.append(Param(pname, _SCALARS[decl], decl, None, False))
            else:
                raise ValueError("%s: parameter `%s` has the unknown type `%s`" % (name, pname, decl))
        protos[name] = Proto(name, _RETURNS[ret], tuple(params))
    return protos, int(abi.group(1)) if abi else None


# One argument of a generated launcher.  A tensor is checked (dtype, device, contiguity) and gives its address; None, an int and a ctypes
# object go to ctypes as they are.
_POINTER = "({a}.data_ptr() if {dtype}{a}.is_cuda and {a}.is_contiguous() else _refuse({i}, {a})) if isinstance({a}, Tensor) else {a}"


def bind(proto, fn):
    """The launcher of one launch entry point, `avc_x(<the header's parameters before the stream>, *, stream=None)`, written out and compiled
    here, once: one expression per argument, so that a call runs no loop and makes no Python call per argument, and Python itself refuses a
    wrong argument count.  This is the cost of a launch on the host (profiles/abi_one_declaration.md)."""
    params = proto.params[:-1]

    def _refuse(i, v):
        q, ok = params[i], _ELEMENTS[params[i].elem]
        if ok is not None and v.dtype not in ok:
            raise TypeError("libavc %s: `%s` is declared `%s`, got a %s tensor" % (proto.name, q.name, q.decl, v.dtype))
        raise ValueError("libavc %s: `%s` (`%s`) needs a contiguous device tensor, got a %s tensor on %s with strides %s"
                         % (proto.name, q.name, q.decl, v.dtype, v.device, tuple(v.stride())))

    def _failed():
        raise RuntimeError("libavc %s failed: %s" % (proto.name, load().avc_last_error().decode()))

    env = {"_fn": fn, "_refuse": _refuse, "_failed": _failed, "Tensor": torch.Tensor, "_current_stream": torch.cuda.current_stream}
    names, exprs = [], []
    for i, q in enumerate(params):
        a = q.name + "_"                       # (never a Python keyword, never one of the names above)
        names.append(a)
        if q.ctype is c_void_p:
            env["_ok%d" % i] = _ELEMENTS[q.elem]
            exprs.append(_POINTER.format(a=a, i=i, dtype="" if _ELEMENTS[q.elem] is None else "%s.dtype in _ok%d and " % (a, i)))
        else:
            exprs.append(a)
    exprs.append("_current_stream().cuda_stream if stream is None else stream")
    exec("def %s(%s*, stream=None):\n    if _fn(%s) != 0:\n        _failed()\n"
         % (proto.name, "".join(n + ", " for n in names), ",\n           ".join(exprs)), env)
    return env[proto.name]


def lib_path():
    return _build.LIB


def load():
    global _lib, ABI_VERSION
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("libavc.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                           "there is no CPU fallback for the HIP hot path")
    protos, declared_in = {}, {}
    for header in headers() + added_headers() + later_headers():
        with open(header) as f:
            more, abi = parse_header(f.read())
        if header == HEADER:
            ABI_VERSION = abi
        twice = sorted(set(more) & set(protos))
        if twice:
            raise RuntimeError("%s declares %s, which %s declares already" % (header, ", ".join(twice), declared_in[twice[0]]))
        protos.update(more)
        declared_in.update((name, header) for name in more)
    lib = ctypes.CDLL(path)
    got = lib.avc_version()
    if got != ABI_VERSION:
        raise RuntimeError("%s implements revision %d of include/avc.h, this binding expects %s: rebuild the library "
                           "(python -m avatarclip_amd.build --force)" % (path, got, ABI_VERSION))
    for name, proto in protos.items():
        fn = getattr(lib, name, None)
        if fn is None:                                   # an added entry point does not change the revision: a library from before it
            where = ("include/" if declared_in[name] == HEADER else "csrc/") + os.path.basename(declared_in[name])
            raise RuntimeError("%s implements revision %d of include/avc.h but lacks %s of %s: rebuild the library "
                               "(python -m avatarclip_amd.build --force)" % (path, got, name, where))
        fn.restype = proto.restype
        fn.argtypes = proto.argtypes
    _launches.update((name, bind(proto, getattr(lib, name))) for name, proto in protos.items() if proto.launch)
    _lib = lib
    return lib


def call(name, *args, stream=None):
    """Launch entry point `name` with `args` in the header's order, without the trailing stream (None: torch's current stream).  A
    non-zero status raises with avc_last_error()."""
    if _lib is None:
        load()
    try:
        launch = _launches[name]
    except KeyError:
        raise AttributeError("include/avc.h, csrc/avc_texture.h and csrc/avc_codebook.h declare no launch entry point %s" % name) from None
    launch(*args, stream=stream)


def ptr(t):
    """device pointer of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "HIP kernels need contiguous device tensors"
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("libavc %s failed: %s" % (what, load().avc_last_error().decode()))
