"""neural_renderer's textured .obj loader, restated on the host: `nr.load_obj(path, load_texture=True, texture_size=ts)` and its
`load_textures` kernel, which AvatarAnimate/models/render.py:6-35 and AvatarGen/ShapeGen/utils.py:6-28 call on data/smpl_uv.obj before every
render.  One-off per run: 13 776 faces x 512 texels is milliseconds of numpy, nothing per iteration; the
per-pixel sampling of the cubes is csrc/avc_raster_tex.hip (mesh_render.render_rgb_batch).  Rules in DESIGN.md section 8; unpinned against
neural_renderer itself.

  parsing   `v`, `vt`, `f a/b[/c] ...` (a polygon is fan-triangulated (0, i+1, i+2), vertex and vt indices alike), `mtllib` (the .mtl, relative
            to the .obj), `usemtl` (the material of the faces that follow).  A material is `Kd r g b` alone (its faces' cubes are that colour) or
            `map_Kd file` (relative to the .obj; read as RGB, float32 / 255, flipped vertically).  Faces before any `usemtl` keep 0.5.
  sampling  texel (i0, i1, i2) of a face: d_k = i_k / (ts - 1), divided by d0 + d1 + d2 where that is > 0; the face's uv corners wrapped
            `mod 1`; pos_x = ((u0 d0 + u1 d1) + u2 d2) (W - 1), pos_y with v and H - 1; x0 = (int)pos_x, x1 = min(x0 + 1, W - 1), weight of x1 =
            pos_x - x0, of x0 = 1 - that, y likewise; colour = the four pixels (y0,x0), (y1,x0), (y0,x1), (y1,x1) times (weight_x * weight_y),
            added in that order.  All in float32.
"""
import os

import numpy as np

f32 = np.float32
UNASSIGNED = 0.5          # the value neural_renderer's cubes start from


def _index(token, count, path, line_no):
    """one 1-based (or negative, relative) .obj index -> 0-based"""
    i = int(token)
    i = i - 1 if i > 0 else count + i
    if not 0 <= i < count:
        raise ValueError("%s:%d: index %s is outside the %d elements read so far" % (path, line_no, token, count))
    return i


def read_mtl(path, obj_path):
    """-> {material: ('Kd', [r, g, b] float32) or ('map_Kd', image path relative to the .obj's folder)}"""
    if not os.path.isfile(path):
        raise ValueError("%s: its material file %s does not exist" % (obj_path, path))
    kd, maps, name = {}, {}, None
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t or t[0].startswith("#"):
                continue
            if t[0] == "newmtl":
                name = t[1]
            elif t[0] == "Kd" and name is not None:
                kd[name] = np.array([float(x) for x in t[1:4]], f32)
            elif t[0] == "map_Kd" and name is not None:
                maps[name] = os.path.join(os.path.dirname(obj_path), t[1])
    return {m: ("map_Kd", maps[m]) if m in maps else ("Kd", kd[m]) for m in list(kd) + [m for m in maps if m not in kd]}


def read_image(path, obj_path):
    """[H,W,3] float32 in [0,1], flipped vertically (row 0 = the image's bottom row: v = 0)"""
    from PIL import Image
    if not os.path.isfile(path):
        raise ValueError("%s: its texture image %s does not exist" % (obj_path, path))
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB")).astype(f32) / f32(255)
    return np.ascontiguousarray(a[::-1])


def sample_cubes(image, uv, texture_size):
    """the texture cubes [F,ts,ts,ts,3] of faces with uv corners [F,3,2] from image [H,W,3] (module docstring: sampling)"""
    ts = int(texture_size)
    H, W = image.shape[:2]
    k = np.arange(ts, dtype=f32) / f32(ts - 1)
    d0, d1, d2 = np.meshgrid(k, k, k, indexing="ij")
    s = (d0 + d1) + d2
    pos = s > 0
    one = np.where(pos, s, f32(1))
    d0, d1, d2 = (np.where(pos, d / one, d).astype(f32)[None] for d in (d0, d1, d2))
    uv = np.mod(np.asarray(uv, f32), f32(1))
    u, v = (uv[:, :, j][:, :, None, None, None] for j in (0, 1))
    pos_x = ((u[:, 0] * d0 + u[:, 1] * d1) + u[:, 2] * d2) * f32(W - 1)
    pos_y = ((v[:, 0] * d0 + v[:, 1] * d1) + v[:, 2] * d2) * f32(H - 1)
    x0, y0 = pos_x.astype(np.int32), pos_y.astype(np.int32)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx1, wy1 = pos_x - x0.astype(f32), pos_y - y0.astype(f32)
    wx0, wy0 = f32(1) - wx1, f32(1) - wy1
    c = image[y0, x0] * (wx0 * wy0)[..., None]
    c = c + image[y1, x0] * (wx0 * wy1)[..., None]
    c = c + image[y0, x1] * (wx1 * wy0)[..., None]
    c = c + image[y1, x1] * (wx1 * wy1)[..., None]
    return c.astype(f32)


def load_obj_texture(path, texture_size=8):
    """-> (vertices [V,3] float32, faces [F,3] int32, textures [F,ts,ts,ts,3] float32), numpy.  ValueError naming the file: texture_size < 2,
    no or a missing .mtl, a missing image, an unknown material, a face without vt under a map_Kd material."""
    ts = int(texture_size)
    if ts < 2:
        raise ValueError("%s: texture_size = %d; a texture cube needs at least 2 texels per axis (the renderer blends texel i with i + 1)" % (path, ts))
    if not os.path.isfile(path):
        raise ValueError("%s does not exist" % path)
    v, vt, faces, face_vt, face_mtl = [], [], [], [], []
    mtl_file, material = None, None
    with open(path) as fh:
        for line_no, line in enumerate(fh, 1):
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:4]])
            elif t[0] == "vt":
                vt.append([float(x) for x in t[1:3]])
            elif t[0] == "mtllib":
                mtl_file = os.path.join(os.path.dirname(path), t[1])
            elif t[0] == "usemtl":
                material = t[1]
            elif t[0] == "f":
                corners = [c.split("/") for c in t[1:]]
                vi = [_index(c[0], len(v), path, line_no) for c in corners]
                ti = [_index(c[1], len(vt), path, line_no) if len(c) > 1 and c[1] else -1 for c in corners]
                for i in range(len(corners) - 2):
                    faces.append([vi[0], vi[i + 1], vi[i + 2]])
                    face_vt.append([ti[0], ti[i + 1], ti[i + 2]])
                    face_mtl.append(material)
    if mtl_file is None:
        raise ValueError("%s names no material file (mtllib): it has no texture to load" % path)
    materials = read_mtl(mtl_file, path)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    face_vt = np.asarray(face_vt, np.int64).reshape(-1, 3)
    vt = np.asarray(vt, f32).reshape(-1, 2)
    textures = np.full((len(faces), ts, ts, ts, 3), UNASSIGNED, f32)
    for name in sorted({m for m in face_mtl if m is not None}):
        if name not in materials:
            raise ValueError("%s uses the material %s, which %s does not define" % (path, name, mtl_file))
        sel = np.array([m == name for m in face_mtl])
        kind, what = materials[name]
        if kind == "Kd":
            textures[sel] = what
            continue
        if (face_vt[sel] < 0).any():
            bad = int(np.nonzero(sel & (face_vt < 0).any(1))[0][0])
            raise ValueError("%s: face %d has no vt index, but its material %s is an image (map_Kd)" % (path, bad, name))
        textures[sel] = sample_cubes(read_image(what, path), vt[face_vt[sel]], ts)
    return np.asarray(v, f32).reshape(-1, 3), faces, textures


def as_cubes(texture, device):
    """AnimateContext's / the CLI's `texture` argument -> the cubes as a float32 tensor on `device`: a tensor [F,ts,ts,ts,3] as it is, a path
    through load_obj_texture (texture_size 8, the reference's)"""
    import torch
    if isinstance(texture, (str, os.PathLike)):
        texture = torch.from_numpy(load_obj_texture(os.fspath(texture))[2])
    if not torch.is_tensor(texture) or texture.dim() != 5 or texture.shape[-1] != 3 or len(set(texture.shape[1:4])) != 1:
        raise ValueError("a texture is the path of an .obj or a tensor of cubes [F,ts,ts,ts,3], got %s"
                         % (list(texture.shape) if torch.is_tensor(texture) else type(texture).__name__))
    return texture.detach().to(device=device, dtype=torch.float32).contiguous()
