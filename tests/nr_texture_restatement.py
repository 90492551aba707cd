"""CPU restatement of neural_renderer's texture path (TEST INFRASTRUCTURE ONLY), in numpy float32 following the rules of DESIGN.md section 8
operation by operation: the textured .obj loader (avatarclip_amd/texture.py is tested against it), the per-pixel sampling of the texture cubes
and the pooled RGB image (csrc/avc_raster_tex.hip), and the approximate backward with the three-channel colour term.  Written from the rules,
not from the code under test: the loader here walks face by face and texel by texel with scalars, the one under test is vectorised.  Unpinned
against neural_renderer itself.

The winner of every pixel is an INPUT here (the face-index map): coverage and depth are the grey kernels' business, pinned by
tests/test_gpu_raster_grad.py.  The backward's scan-line walk is tests/nr_grad_restatement.walk, the one pseudo_grad runs with the grey
colour term: this module holds only the three-channel hook (rgb_delta) and its maps.  The barycentrics are R.face_weights, the rasteriser's.
"""
import os

import numpy as np

from tests import nr_grad_restatement as R

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------------ the loader
def _parse(path):
    v, vt, faces, fvt, fm, mtllib, cur = [], [], [], [], [], None, None
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "v":
            v.append([float(x) for x in t[1:4]])
        elif t[0] == "vt":
            vt.append([float(x) for x in t[1:3]])
        elif t[0] == "mtllib":
            mtllib = t[1]
        elif t[0] == "usemtl":
            cur = t[1]
        elif t[0] == "f":
            c = [x.split("/") for x in t[1:]]
            for i in range(len(c) - 2):                      # fan (0, i+1, i+2)
                tri = (c[0], c[i + 1], c[i + 2])
                faces.append([int(x[0]) - 1 for x in tri])
                fvt.append([int(x[1]) - 1 if len(x) > 1 and x[1] else None for x in tri])
                fm.append(cur)
    return np.array(v, f32), vt, np.array(faces, np.int32), fvt, fm, mtllib


def _materials(path):
    out, cur = {}, None
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "newmtl":
            cur = t[1]
            out[cur] = {}
        elif t[0] in ("Kd", "map_Kd"):
            out[cur][t[0]] = t[1:]
    return out


def texel(image, uv, i, ts):
    """one texel (i0, i1, i2) of a face with uv corners uv [3][2] from image [H,W,3] (already flipped): scalar float32, in the rules' order"""
    H, W = image.shape[:2]
    d = [f32(i[k]) / f32(ts - 1) for k in range(3)]
    s = f32(f32(d[0] + d[1]) + d[2])
    if s > 0:
        d = [f32(x / s) for x in d]
    u = [f32(np.fmod(f32(c[0]), f32(1))) for c in uv]
    v = [f32(np.fmod(f32(c[1]), f32(1))) for c in uv]
    u = [x + f32(1) if x < 0 else x for x in u]              # `mod 1` with the sign of the divisor (REPEAT)
    v = [x + f32(1) if x < 0 else x for x in v]
    pos_x = f32(f32(f32(u[0] * d[0]) + f32(u[1] * d[1])) + f32(u[2] * d[2])) * f32(W - 1)
    pos_y = f32(f32(f32(v[0] * d[0]) + f32(v[1] * d[1])) + f32(v[2] * d[2])) * f32(H - 1)
    x0, y0 = int(pos_x), int(pos_y)
    x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
    wx1, wy1 = f32(pos_x - f32(x0)), f32(pos_y - f32(y0))
    wx0, wy0 = f32(f32(1) - wx1), f32(f32(1) - wy1)
    c = image[y0, x0] * f32(wx0 * wy0)
    c = c + image[y1, x0] * f32(wx0 * wy1)
    c = c + image[y0, x1] * f32(wx1 * wy0)
    c = c + image[y1, x1] * f32(wx1 * wy1)
    return c.astype(f32)


def load_obj_texture(path, ts=8):
    """the loader's rules -> (vertices, faces, textures [F,ts,ts,ts,3])"""
    from PIL import Image
    v, vt, faces, fvt, fm, mtllib = _parse(path)
    here = os.path.dirname(path)
    mats = _materials(os.path.join(here, mtllib))
    images = {}
    tex = np.full((len(faces), ts, ts, ts, 3), 0.5, f32)
    for f in range(len(faces)):
        if fm[f] is None:
            continue
        m = mats[fm[f]]
        if "map_Kd" not in m:
            tex[f] = np.array([float(x) for x in m["Kd"][:3]], f32)
            continue
        name = m["map_Kd"][0]
        if name not in images:
            images[name] = (np.asarray(Image.open(os.path.join(here, name)).convert("RGB")).astype(f32) / f32(255))[::-1]
        uv = [vt[j] for j in fvt[f]]
        for i0 in range(ts):
            for i1 in range(ts):
                for i2 in range(ts):
                    tex[f, i0, i1, i2] = texel(images[name], uv, (i0, i1, i2), ts)
    return v, faces, tex


# ------------------------------------------------------------------------------------------------------------------- the per-pixel sample
def weights(tri, xs, ys, n):
    """R.face_weights at the integer pixels (xs, ys) of an n x n grid for a face's NDC vertices tri [3,3]"""
    return R.face_weights(R.pixel_coords(tri, n), tri[:, 2], np.asarray(xs).astype(f32), np.asarray(ys).astype(f32))


def cube_of(textures, f):
    """the cube face f of a face list [faces; reversed copies] samples: a fill-back copy reads its face's cube with axes 0 and 2 swapped"""
    Ft = textures.shape[0]
    return textures[f] if f < Ft else textures[f - Ft].transpose(2, 1, 0, 3)


def blend(cube, w, ws, zp, z, eps=1e-4):
    """the unlit colours [P,3] of pixels with clamped weights w [3,P], their sum ws, depth zp, of a face with vertex depths z [3]"""
    ts = cube.shape[0]
    i, r = [], []
    for k in range(3):
        t = w[k] / ws * f32(ts - 1) * (zp / z[k])
        t = np.minimum(np.maximum(t, f32(0)), f32(ts - 1) - f32(eps))
        ik = t.astype(np.int64)
        i.append(ik)
        r.append((t - ik.astype(f32)).astype(f32))
    U = np.zeros((w.shape[1], 3), f32)
    for pn in range(8):
        b = [(pn >> k) & 1 for k in range(3)]
        m = [r[k] if b[k] else f32(1) - r[k] for k in range(3)]
        wt = (m[0] * m[1]) * m[2]
        U = U + wt[:, None] * cube[i[0] + b[0], i[1] + b[1], i[2] + b[2]]
    return U.astype(f32)


def unlit_map(ndc, faces2, fidx, textures, eps=1e-4):
    """U of every super-sampled pixel from the face-index map [n,n] (y up, -1: background -> 0) -> [n,n,3]"""
    nd, tex = np.asarray(ndc, f32), np.asarray(textures, f32)
    n = fidx.shape[0]
    U = np.zeros((n, n, 3), f32)
    for f in np.unique(fidx[fidx >= 0]):
        ys, xs = np.nonzero(fidx == f)
        tri = nd[np.asarray(faces2)[f]]
        with np.errstate(divide="ignore", invalid="ignore"):
            w, ws, zp = weights(tri, xs, ys, n)
            U[ys, xs] = blend(cube_of(tex, int(f)), w, ws, zp, tri[:, 2], eps)
    return U


def lit_map(unlit, fidx, light):
    """C = light[I] U (0 on background) [n,n,3]"""
    lt = np.asarray(light, f32)
    l = np.where(fidx >= 0, lt[np.maximum(fidx, 0)], f32(0))
    return (l[..., None] * unlit).astype(f32)


def pooled_image(unlit, fidx, light):
    """the forward's image [S,S,3]: lit colours, rows flipped, 2 x 2 average ((a + b) + c) + d, / 4"""
    c = lit_map(unlit, fidx, light)[::-1]
    S = c.shape[0] // 2
    c4 = c.reshape(S, 2, S, 2, 3)
    return (((c4[:, 0, :, 0] + c4[:, 0, :, 1]) + c4[:, 1, :, 0]) + c4[:, 1, :, 1]) / f32(4)


# --------------------------------------------------------------------------------------------------------------------------- the backward
def G_map3(grad_image):
    """G_c at the super-sampled pixels [n,n,3], y up, from grad_image [S,S,3]"""
    g = np.asarray(grad_image, f32)[::-1]
    return np.repeat(np.repeat(g, 2, 0), 2, 1) * f32(0.25)


def rgb_delta(C, G):
    """the textured colour term: sum over c ascending of (C_c(w) - C_c(w_ref)) G_c(w)"""
    def fn(px, ref):
        d = (C[px] - C[ref]) * G[px]
        return ((d[..., 0] + d[..., 1]) + d[..., 2]).astype(f32)
    return fn


def backward(ndc, faces2, light, fidx, unlit, grad_image, eps=1e-4, abs_sum=None):
    """grad_image [S,S,3] -> (grad_ndc [V,3], grad_light [F] = sum over the face's pixels of sum_c G_c U_c)"""
    fidx = np.asarray(fidx)
    G = G_map3(grad_image)
    C = lit_map(np.asarray(unlit, f32), fidx, light)
    gn = R.walk(ndc, faces2, fidx, rgb_delta(C, G), eps, abs_sum=abs_sum)
    gu = G * np.asarray(unlit, f32)
    per_pixel = ((gu[..., 0] + gu[..., 1]) + gu[..., 2]).astype(np.float64)
    m = fidx >= 0
    return gn, np.bincount(fidx[m], weights=per_pixel[m], minlength=len(faces2))
