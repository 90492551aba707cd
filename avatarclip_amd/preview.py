"""Look at what the pipeline writes: a turn-table or a played motion of a .ply, a .ply + .pc2, a .glb, or of the SMPL body in the poses
animate writes, as a GIF or a PNG.

    python -m avatarclip_amd.preview (--mesh X.ply [--pc2 M.pc2] | --glb X.glb | --smpl SMPL.npz --poses X.npy) --out P.gif|P.png
                                     [--views 36] [--size 512] [--ss 2] [--up y|z] [--elevation deg] [--fov deg]
                                     [--fps 30] [--every k] [--frames-dir D] [--orbit]
                                     [--focus head|upper|lower|LO:HI] [--eye X Y Z --at X Y Z] [--clip]

A static source (a .ply alone, a .glb without a track, one pose) makes a turn-table of --views frames; a moving one (a .pc2, a .glb with a
track, a motion of more than one pose) plays its frames from the fixed front camera, or from a camera that goes round once with --orbit.
A .png takes the first frame.  --smpl / --poses pose the SMPL body itself (smpl_lbs.pose_hip, csrc/avc_smpl.hip) in animate's
candidate_<i>.npy or motion.npy: the uncoloured grey body, y up, facing +z, the root rotation dropped as the reference's previews drop it
(AvatarAnimate/visualize.py:98-102, :115-119), under frame_cameras' auto-framed camera -- NOT pyrender's fixed camera of f = 5000.  --up is
the axis that points up in the file: y for Runner.validate_mesh's .ply and for rig's .glb (SMPL's frame), z for drive's outputs (drive
rotates into Blender's frame), which is the default as soon as --pc2 is given.  A .glb that rig wrote WITH --motion (and without
--keep_root) also plays in Blender's frame, because its tracks carry drive's root rotation (pi/2, 0, 0): give --up z for it (rig --preview
does); its rest pose is y up.

The reference renders its results through pyrender and OSMesa (AvatarAnimate/visualize.py: render_pose, render_motion); this is a renderer
of this project's own (csrc/avc_preview.hip: exact integer coverage and depth, top-left fill rule, vertex colours, flat two-sided shading
with a headlight), not a port of that one.  A FACE WITH A VERTEX NEARER THAN `near`, BEYOND `far` OR OUTSIDE THE GUARD BAND OF 256 RASTER
PIXELS AROUND THE IMAGE IS DROPPED, NOT CLIPPED, UNLESS `clip`.  frame_cameras' whole-mesh cameras never produce one; a close-up does:
--focus frames a band of the mesh's height (head = 0.84:1, upper = 0.5:1, lower = 0:0.5, or LO:HI), --eye / --at place one fixed camera
by hand, and both (like --clip alone) turn the frustum clipper on (csrc/avc_preview_clip.hip: such a face is cut at near, far and the four
sides one raster pixel outside the guard band, and what is left is drawn under the face's own index), so the shoulders run out of a
picture of the head instead of going missing.  Without these options every picture is bit for bit what it was."""
import argparse
import math
import os

import numpy as np
import torch

from . import drive
from . import lib as L
from . import mesh as _mesh
from . import rig

MAX_RASTER = 2048                         # AVC_PREVIEW_MAX_RASTER: image_size * ss
CHUNK_BYTES = 256 << 20                   # device memory of one chunk of frames (z-buffer keys, projected vertices, images)
GREY = 200.0                              # the colour of a mesh without colours
_UP = {"y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0)}
_FRONT = {"y": (0.0, 0.0, 1.0), "z": (0.0, -1.0, 0.0)}   # where the avatar looks: +z in SMPL's frame, -y after drive's (x, y, z) -> (x, -z, y)
FOCUS = {"head": (0.84, 1.0), "upper": (0.5, 1.0), "lower": (0.0, 0.5)}   # --focus: bands of the mesh's extent along `up`


def _up_vector(up):
    if up not in _UP:
        raise ValueError("up is 'y' or 'z', got %r" % (up,))
    return np.asarray(_UP[up], np.float64)


# ---------------------------------------------------------------------------------------------------------------- cameras
def look_frames(eyes, ats, up):
    """cams float32 [N,12] = eye, x (right), y (up), z (forward) of a right-handed look-at: z = (at - eye) / |.|, x = z x up / |.|, y = x x z.
    The layout avc_rasterize_mesh takes (NOT neural_renderer's mirrored x axis)."""
    eyes, ats = np.asarray(eyes, np.float64).reshape(-1, 3), np.asarray(ats, np.float64).reshape(-1, 3)
    ats = np.broadcast_to(ats, eyes.shape)
    z = ats - eyes
    z = z / np.linalg.norm(z, axis=1, keepdims=True)
    x = np.cross(z, _up_vector(up)[None])
    if np.any(np.linalg.norm(x, axis=1) < 1e-9):
        raise ValueError("a camera looks along the up axis")
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    y = np.cross(x, z)
    return np.concatenate([eyes, x, y, z], 1).astype(np.float32)


def bounding_sphere(vertices):
    """(centre [3], radius) of all frames as Python floats: the centre of the bounding box and the largest distance from it, computed
    where the vertices live"""
    v = vertices.reshape(-1, 3)
    mn, mx = torch.aminmax(v, dim=0)
    c = (mn + mx) * 0.5
    r = torch.linalg.norm(v - c[None], dim=1).max()
    return c.double().cpu().numpy(), float(r)


def depth_range(vertices, eyes):
    """(near, far) of the whole bounding sphere of `vertices` seen from `eyes` [n,3], near floored at far * 1e-3: render_frames' default"""
    ctr, rad = bounding_sphere(vertices)
    dist = np.linalg.norm(np.asarray(eyes, np.float64).reshape(-1, 3) - ctr[None], axis=1)
    far = float(dist.max() + rad) * 1.01
    return max(float(dist.min() - rad) * 0.99, far * 1e-3), far


def parse_focus(text):
    """'head' | 'upper' | 'lower' | 'LO:HI' -> (lo, hi) with 0 <= lo < hi <= 1"""
    if text in FOCUS:
        return FOCUS[text]
    try:
        lo, hi = (float(x) for x in str(text).split(":"))
    except ValueError:
        raise ValueError("--focus is head, upper, lower or LO:HI, got %r" % (text,)) from None
    if not 0.0 <= lo < hi <= 1.0:
        raise ValueError("--focus LO:HI needs 0 <= LO < HI <= 1, got %r" % (text,))
    return lo, hi


def frame_cameras(vertices, n_views=36, elevation=10.0, up="y", fov=40.0, margin=0.05, focus=None):
    """Auto-framed cameras: n_views eyes on a circle around the `up` axis through the centre of the bounding sphere of ALL frames
    (vertices [N,V,3] or [V,3], tensor or array), `elevation` degrees above the horizon, at the distance at which the sphere's outline
    stays `margin` (a fraction of the half image) inside the field of view `fov` (degrees, full angle).  View 0 is the front view.
    Returns (eyes [n,3], ats [n,3], near, far) with every vertex strictly between near and far for each of the cameras.
    focus = (lo, hi), 0 <= lo < hi <= 1, frames a BAND of the mesh instead: the sphere is that of the vertices (of all frames) whose
    coordinate along `up` lies in that fraction of the mesh's extent along `up` (none: a ValueError); near and far still come from the
    WHOLE mesh (depth_range: a hand in front of the face is not cut away, near floored at far * 1e-3), so the rest of the mesh runs out of
    the picture -- render such cameras with render_frames(clip=True)."""
    v = vertices if torch.is_tensor(vertices) else torch.as_tensor(np.asarray(vertices, np.float32))
    if v.numel() == 0 or v.shape[-1] != 3:
        raise ValueError("frame_cameras takes [N, V, 3] or [V, 3] vertices, V > 0")
    if not 0.0 <= margin < 1.0 or not 0.0 < fov < 180.0 or n_views < 1:
        raise ValueError("frame_cameras: margin in [0, 1), fov in (0, 180), n_views >= 1")
    v = v.to(torch.float32)
    band = v
    if focus is not None:
        lo, hi = (float(x) for x in focus)
        if not 0.0 <= lo < hi <= 1.0:
            raise ValueError("frame_cameras: focus = (lo, hi) with 0 <= lo < hi <= 1, got %r" % (focus,))
        h = v.reshape(-1, 3)[:, int(np.argmax(_up_vector(up)))]
        h0, h1 = (float(x) for x in torch.aminmax(h))
        band = v.reshape(-1, 3)[(h >= h0 + lo * (h1 - h0)) & (h <= h0 + hi * (h1 - h0))]
        if band.shape[0] == 0:
            raise ValueError("frame_cameras: no vertex lies in the band %g:%g of the mesh's height" % (lo, hi))
    c, r = bounding_sphere(band)
    r = max(r, 1e-6)
    # the outline of a sphere at distance d is a circle of tan(asin(r / d)) around the image centre
    d = r / math.sin(math.atan((1.0 - margin) * math.tan(math.radians(fov) * 0.5)))
    u = _up_vector(up)
    f = np.asarray(_FRONT[up], np.float64)
    s = np.cross(u, f)
    a = 2.0 * np.pi * np.arange(n_views) / n_views
    el = math.radians(elevation)
    dirs = math.cos(el) * (np.cos(a)[:, None] * f[None] + np.sin(a)[:, None] * s[None]) + math.sin(el) * u[None]
    eyes = c[None] + d * dirs
    ats = np.broadcast_to(c[None], eyes.shape).copy()
    if focus is not None:
        return (eyes, ats) + depth_range(v, eyes)
    return eyes, ats, (d - r) * 0.99, (d + r) * 1.01


# ---------------------------------------------------------------------------------------------------------------- the renderer
def check_raster(image_size, ss):
    if ss not in (1, 2):
        raise ValueError("ss (supersampling) is 1 or 2, got %s" % (ss,))
    if image_size < 1 or image_size * ss > MAX_RASTER:
        raise ValueError("image_size * ss = %d is outside [1, %d], the raster the kernel's int64 arithmetic is proven for"
                         % (image_size * ss, MAX_RASTER))


def scratch_bytes(num_faces, raster_size):
    """avc_preview_scratch_bytes: the bytes of z-buffer keys and large-face list one frame needs"""
    return int(L.load().avc_preview_scratch_bytes(int(num_faces), int(raster_size)))


def render_frames(vertices, triangles, colors=None, eyes=None, ats=None, up="y", fov=40.0, image_size=512, ss=2, light=None, ambient=0.4,
                  background=(255, 255, 255), return_face_ids=False, near=None, far=None, chunk_bytes=CHUNK_BYTES, scratch=None, clip=False,
                  texture=None):
    """uint8 [N,S,S,3] device tensor (row 0 = top) of N frames of ONE topology.  vertices [N,V,3] (or [V,3]: the same mesh for every
    camera), triangles [F,3], colors uint8 [V,3|4] or None (a constant grey) -- device tensors or arrays; eyes / ats [N,3] (or [3]);
    light [N,3] or [3] direction, None = a headlight (at - eye).  near / far default to the range of the frames' bounding sphere seen from
    the eyes.  With return_face_ids also int32 [N, S ss, S ss], the winning face of every raster pixel (-1: background).  Frames are
    rendered in chunks of at most chunk_bytes of device memory.  Faces with a vertex outside (near, far] or the guard band are dropped;
    with clip=True they are clipped at the frustum instead (avc_preview_raster_clip / avc_preview_shade_clip) and every other face is
    drawn bit for bit as without it.
    scratch: a uint8 device tensor of at least scratch_bytes(F, S ss) bytes, all 0xFF, to use instead of a fresh one (it comes back all
    0xFF).
    texture = (uv float32 [V,2], image uint8 [T,T,3]) instead of colors: the colour is a bilinear, clamp-to-edge fetch at the
    perspective-correct UV (avc_preview_shade_tex; a rig --bake_texture .glb).  The clipped path has no textured variant: clip=True with a
    texture is a ValueError."""
    if texture is not None and clip:
        raise ValueError("render_frames: the clipped path has no textured variant yet (csrc/avc_preview_clip.hip interpolates vertex colours "
                         "only): give clip=True or a texture, not both")
    if texture is not None and colors is not None:
        raise ValueError("render_frames: give colors or a texture, not both")
    check_raster(int(image_size), int(ss))
    S, ss = int(image_size), int(ss)
    R = S * ss
    dev = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device("cuda")
    v = (vertices if torch.is_tensor(vertices) else torch.as_tensor(np.asarray(vertices, np.float32))).to(device=dev, dtype=torch.float32)
    if v.dim() == 2:
        v = v[None]
    if v.dim() != 3 or v.shape[2] != 3:
        raise ValueError("vertices must be [N, V, 3] or [V, 3], got %s" % (tuple(v.shape),))
    V = v.shape[1]
    t = drive._i32(triangles, dev).reshape(-1, 3)
    F = t.shape[0]
    if F and (V == 0 or int(t.min()) < 0 or int(t.max()) >= V):
        raise ValueError("a triangle names a vertex outside [0, %d)" % V)
    c = None
    if colors is not None:
        c = torch.as_tensor(np.asarray(colors) if not torch.is_tensor(colors) else colors)
        if c.dim() != 2 or c.shape[0] != V or c.shape[1] not in (3, 4) or c.dtype != torch.uint8:
            raise ValueError("colors must be [V, 3] or [V, 4] uint8, got %s %s" % (tuple(c.shape), c.dtype))
        c = c.to(dev).contiguous()
    uv_d = tex_d = None
    if texture is not None:
        uv_d, tex_d = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)) for x in texture)
        if uv_d.shape != (V, 2) or uv_d.dtype != torch.float32:
            raise ValueError("texture uv must be float32 [V, 2], got %s %s" % (tuple(uv_d.shape), uv_d.dtype))
        if tex_d.dim() != 3 or tex_d.shape[0] != tex_d.shape[1] or tex_d.shape[2] != 3 or tex_d.dtype != torch.uint8 or not 1 <= tex_d.shape[0] <= 4096:
            raise ValueError("texture image must be uint8 [T, T, 3] with T in [1, 4096], got %s %s" % (tuple(tex_d.shape), tex_d.dtype))
        uv_d, tex_d = uv_d.to(dev).contiguous(), tex_d.to(dev).contiguous()
    if eyes is None or ats is None:
        raise ValueError("render_frames needs eyes and ats (frame_cameras gives both)")
    eyes = np.asarray(eyes.cpu() if torch.is_tensor(eyes) else eyes, np.float64).reshape(-1, 3)
    ats = np.asarray(ats.cpu() if torch.is_tensor(ats) else ats, np.float64).reshape(-1, 3)
    N = max(v.shape[0], eyes.shape[0])
    if v.shape[0] not in (1, N) or eyes.shape[0] not in (1, N) or ats.shape[0] not in (1, N):
        raise ValueError("vertices, eyes and ats disagree about the number of frames")
    eyes, ats = np.broadcast_to(eyes, (N, 3)), np.broadcast_to(ats, (N, 3))
    cams = look_frames(eyes, ats, up)
    lights = (ats - eyes) if light is None else np.broadcast_to(np.asarray(light, np.float64).reshape(-1, 3), (N, 3))
    if near is None or far is None:
        near_d, far_d = depth_range(v, eyes) if V else (0.1, 10.0)
        near, far = (near_d if near is None else near), (far_d if far is None else far)
    if not 0.0 < near < far:
        raise ValueError("render_frames needs 0 < near < far")
    width = math.tan(math.radians(fov) * 0.5)
    lib, s = L.load(), L.stream()
    per_scratch = int(lib.avc_preview_scratch_bytes(F, R))
    if per_scratch < 0:
        raise ValueError("avc_preview_scratch_bytes refused F = %d, raster %d" % (F, R))
    per_frame = per_scratch + 28 * V + 3 * S * S + (4 * R * R if return_face_ids else 0)
    n = max(1, min(N, 65535, int(chunk_bytes) // max(1, per_frame)))
    images = torch.empty(N, S, S, 3, device=dev, dtype=torch.uint8)
    ids = torch.empty(N, R, R, device=dev, dtype=torch.int32) if return_face_ids else None
    if scratch is None:
        scratch = torch.full((n * per_scratch,), 255, device=dev, dtype=torch.uint8)     # filled once; every call hands it back that way
    else:
        if scratch.dtype != torch.uint8 or not scratch.is_cuda or scratch.numel() < per_scratch:
            raise ValueError("scratch must be a uint8 device tensor of at least %d bytes" % per_scratch)
        n = min(n, scratch.numel() // per_scratch)
    proj = torch.empty(n, max(V, 1), 4, device=dev, dtype=torch.int32)
    cams_d = torch.from_numpy(cams).to(dev)
    lights_d = torch.from_numpy(np.ascontiguousarray(lights, dtype=np.float32)).to(dev)
    bg = [float(x) for x in background]
    for f0 in range(0, N, n):
        k = min(n, N - f0)
        vk = (v[f0:f0 + k] if v.shape[0] == N else v.expand(k, -1, -1)).contiguous()
        if V:
            L.call("avc_preview_project", vk, k, V, cams_d[f0:f0 + k], width, near, far, R, proj, stream=s)
            if clip:
                L.call("avc_preview_raster_clip", proj, vk, k, V, cams_d[f0:f0 + k], width, near, far, t if F else None, F, R, scratch, stream=s)
            else:
                L.call("avc_preview_raster", proj, k, V, t if F else None, F, R, scratch, stream=s)
        if clip:
            L.call("avc_preview_shade_clip", proj, vk if V else None, k, V, cams_d[f0:f0 + k], width, near, far, t if F else None, F, c,
                   c.shape[1] if c is not None else 0, lights_d[f0:f0 + k], float(ambient), bg[0], bg[1], bg[2], GREY, S, ss, scratch,
                   images[f0:f0 + k], ids[f0:f0 + k] if ids is not None else None, stream=s)
            continue
        if tex_d is not None:
            L.call("avc_preview_shade_tex", proj, vk if V else None, k, V, t if F else None, F, uv_d if V else None, tex_d, tex_d.shape[0],
                   lights_d[f0:f0 + k], float(ambient), bg[0], bg[1], bg[2], S, ss, scratch, images[f0:f0 + k],
                   ids[f0:f0 + k] if ids is not None else None, stream=s)
            continue
        L.call("avc_preview_shade", proj, vk if V else None, k, V, t if F else None, F, c, c.shape[1] if c is not None else 0, lights_d[f0:f0 + k],
               float(ambient), bg[0], bg[1], bg[2], GREY, S, ss, scratch, images[f0:f0 + k], ids[f0:f0 + k] if ids is not None else None, stream=s)
    return (images, ids) if return_face_ids else images


# ---------------------------------------------------------------------------------------------------------------- skinning
def skin_blend4(joints, weights, joint_mats, rest):
    """Linear blend skinning of a glTF skin (avc_skin_blend4, once per set of four influences): joints uint8 [S,M,4] (or [M,4]), weights
    float32 likewise, joint_mats [T,J,3,4] or [T,J,12] float32 (rows 0..2 of the joint matrices), rest [M,3] -> [T,M,3] device tensor"""
    dev = rest.device if torch.is_tensor(rest) and rest.is_cuda else torch.device("cuda")
    as_t = lambda a, dt: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device=dev, dtype=dt).contiguous()
    j, w, r = as_t(joints, torch.uint8), as_t(weights, torch.float32), as_t(rest, torch.float32)
    m = as_t(joint_mats, torch.float32)
    m = m.reshape(m.shape[0], m.shape[1], 12)
    if j.dim() == 2:
        j, w = j[None], w[None]
    T, J, M = m.shape[0], m.shape[1], r.shape[0]
    if j.shape[1:] != (M, 4) or w.shape != j.shape or r.shape != (M, 3):
        raise ValueError("skin_blend4 takes joints / weights [S, M, 4] and rest [M, 3]")
    if M and int(j.max()) >= J:
        raise ValueError("skin_blend4: a joint index outside [0, %d)" % J)
    out = None
    for k in range(j.shape[0]):
        o = torch.empty(T, M, 3, device=dev, dtype=torch.float32)
        L.call("avc_skin_blend4", j[k].contiguous(), w[k].contiguous(), m, r, M, J, T, o)
        out = o if out is None else out + o
    return out


def quat_to_mat(q):
    """[..., 4] (x, y, z, w) -> [..., 3, 3], normalised first"""
    q = q / torch.linalg.norm(q, dim=-1, keepdim=True)
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def glb_joint_matrices(g, every=1):
    """Forward kinematics over the skeleton rig.read_glb returns: float64 torch [T,J,3,4], joint matrix = global transform of the joint's
    node x its inverse bind matrix, for the key frames of the rotation tracks (every `every`-th), or T = 1 at the rest pose without a
    track.  Also returns the times [T] (zeros without a track)."""
    nodes, skin = g["nodes"], g.get("skin")
    if skin is None:
        raise ValueError("the .glb has no skin")
    tracks = {a["node"]: a for a in g["animation"] if a["path"] == "rotation"}
    lengths = {len(a["times"]) for a in tracks.values()}
    if len(lengths) > 1:
        raise ValueError("the rotation tracks have different lengths")
    T = lengths.pop() if lengths else 1
    times = np.asarray(next(iter(tracks.values()))["times"], np.float64) if tracks else np.zeros(1)
    sel = np.arange(0, T, max(1, int(every)))
    glob = {}

    def world(i):
        if i not in glob:
            n = nodes[i]
            q = torch.from_numpy(np.asarray(tracks[i]["values"], np.float64)[sel]) if i in tracks else \
                torch.from_numpy(n["rotation"]).reshape(1, 4).expand(len(sel), 4)
            m = torch.zeros(len(sel), 4, 4, dtype=torch.float64)
            m[:, :3, :3] = quat_to_mat(q)
            m[:, :3, 3] = torch.from_numpy(n["translation"])
            m[:, 3, 3] = 1.0
            glob[i] = m if n["parent"] is None else world(n["parent"]) @ m
        return glob[i]

    ibm = torch.from_numpy(np.asarray(skin["inverse_bind_matrices"], np.float64))
    mats = torch.stack([world(node) @ ibm[k] for k, node in enumerate(skin["joints"])], 1)
    return mats[:, :, :3, :].contiguous(), times[sel]


def glb_skin(g):
    """(rest [M,3] float32, triangles [F,3] int32, colors uint8 [M,4] or None, joints uint8 [S,M,4], weights float32 [S,M,4])"""
    a = g["attributes"]
    sets = sorted(int(k[7:]) for k in a if k.startswith("JOINTS_"))
    if not sets:
        raise ValueError("the .glb's mesh has no JOINTS_0")
    joints = np.stack([a["JOINTS_%d" % s] for s in sets]).astype(np.uint8)
    weights = np.stack([a["WEIGHTS_%d" % s] for s in sets]).astype(np.float32)
    colors = a.get("COLOR_0")
    return (np.asarray(a["POSITION"], np.float32), np.asarray(g["indices"]).reshape(-1, 3).astype(np.int32),
            None if colors is None else np.asarray(colors, np.uint8), joints, weights)


# ---------------------------------------------------------------------------------------------------------------- sources
def mesh_source(ply, pc2=None, every=1):
    """(vertices float32 [T,V,3], triangles, colors uint8 or None, moving): a .ply (T = 1), or its T posed frames from a .pc2 of drive's"""
    v, t, c = _mesh.read_ply(str(ply))
    if pc2 is None:
        return v[None], t, c, False
    head, frames = drive.read_pc2(str(pc2))
    if frames.shape[1] != v.shape[0]:
        raise ValueError("%s holds %d vertices per frame, %s has %d" % (pc2, frames.shape[1], ply, v.shape[0]))
    if frames.shape[0] == 0:
        raise ValueError("%s holds no frame" % pc2)
    return np.ascontiguousarray(frames[::max(1, int(every))], np.float32), t, c, True


def glb_source(glb, every=1, device=None, return_texture=False):
    """(vertices [T,M,3] device tensor, triangles, colors, moving): the skinned mesh of a rig's .glb at the key frames of its track
    (forward kinematics in torch, the blend by avc_skin_blend4), or at the rest pose.  return_texture: a fifth item, render_frames'
    texture = (uv [M,2], image [T,T,3]) of a file with a baked texture, None of one without"""
    g = rig.read_glb(str(glb))
    rest, t, c, joints, weights = glb_skin(g)
    mats, _ = glb_joint_matrices(g, every)
    dev = torch.device(device) if device is not None else torch.device("cuda")
    v = skin_blend4(joints, weights, mats.to(torch.float32).to(dev), torch.from_numpy(rest).to(dev))
    if return_texture:
        return v, t, c, bool(g["animation"]), (None if g["image"] is None else (g["uv"], g["image"]))
    return v, t, c, bool(g["animation"])


def body_pose(array):
    """float32 [T,72] full SMPL poses for a preview, from the layouts drive.read_pose_my accepts: [T, >= 72] (the first 72 values), [T, 69]
    (the body pose without the root: animate's motion.npy), [T, 63] (6 zeros appended: animate's candidate_<i>.npy); a 1-D pose is one
    frame.  The root rotation is set to ZERO, not to drive's (pi/2, 0, 0): the body stands y up and faces +z.  (visualize.py:98-102,
    :115-119 drop the root as well; their global_orient of pi about x and their mesh's turn by 180 degrees about x cancel up to a
    translation, which the auto-framing removes.)  Plain numpy."""
    p = np.array(array.detach().cpu().numpy() if torch.is_tensor(array) else array, dtype=np.float32)
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2 or p.shape[0] == 0 or not (p.shape[1] in (63, 69) or p.shape[1] >= 72):
        raise ValueError("poses are [T, 72], [T, 69] or [T, 63] (or one such pose), got %s" % (p.shape,))
    if p.shape[1] == 63:
        p = np.concatenate([p, np.zeros((p.shape[0], 6), np.float32)], 1)
    if p.shape[1] == 69:
        p = np.concatenate([np.zeros((p.shape[0], 3), np.float32), p], 1)
    p = np.ascontiguousarray(p[:, :72])
    p[:, :3] = 0
    return p


def smpl_source(smpl, poses, every=1, device=None):
    """(vertices [T,V,3] device tensor, faces, None, moving): the SMPL body in the given poses (a .npy path or an array, body_pose's
    layouts), posed by smpl_lbs.pose_hip.  smpl: a path for smpl_lbs.load_smpl_arrays or its dict (with `faces`).  moving = T > 1."""
    from . import smpl_lbs
    p = body_pose(np.load(poses) if isinstance(poses, (str, os.PathLike)) else poses)[::max(1, int(every))]
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if isinstance(smpl, (str, os.PathLike)):
        a = smpl_lbs.load_smpl_arrays(str(smpl), dev)
    else:                                     # (pose_hip works where the arrays live; a device given here moves them first)
        a = smpl if device is None else {k: (x.to(dev) if torch.is_tensor(x) and k != "parents" else x) for k, x in smpl.items()}
    if "faces" not in a:
        raise ValueError("the SMPL arrays hold no faces")
    v = smpl_lbs.pose_hip(a, torch.from_numpy(np.ascontiguousarray(p)))
    faces = a["faces"]
    faces = np.asarray(faces.cpu() if torch.is_tensor(faces) else faces).reshape(-1, 3).astype(np.int32)
    return v, faces, None, p.shape[0] > 1


# ---------------------------------------------------------------------------------------------------------------- files
def save_frames(images, out, fps=30.0, frames_dir=None):
    """uint8 [N,S,S,3] -> an animated GIF (all frames) or a PNG (the first); frames_dir: numbered PNGs of every frame as well"""
    from PIL import Image
    a = images.cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    frames = [Image.fromarray(np.ascontiguousarray(f)) for f in a]
    ext = os.path.splitext(out)[1].lower()
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    if ext == ".gif":
        frames[0].save(out, save_all=True, append_images=frames[1:], duration=max(1, int(round(1000.0 / fps))), loop=0)
    elif ext == ".png":
        frames[0].save(out)
    else:
        raise ValueError("--out ends in .gif or .png, got %r" % out)
    if frames_dir:
        os.makedirs(frames_dir, exist_ok=True)
        for i, f in enumerate(frames):
            f.save(os.path.join(frames_dir, "%04d.png" % i))
    return out


def preview(out, mesh=None, pc2=None, glb=None, views=36, size=512, ss=2, up=None, elevation=10.0, fov=40.0, fps=30.0, every=1,
            frames_dir=None, orbit=False, margin=0.05, smpl=None, poses=None, focus=None, eye=None, at=None, clip=False):
    """The whole tool: one source -> frames -> a file.  Returns (out, images).  focus: a band for frame_cameras (a name of FOCUS, 'LO:HI'
    or a pair); eye + at: one hand-placed fixed camera for every frame (a static source: one frame); either, or clip, turns clipping on."""
    if (smpl is None) != (poses is None):
        raise ValueError("--smpl and --poses go together: the SMPL model and the poses to put it in")
    if (mesh is not None) + (glb is not None) + (smpl is not None) != 1:
        raise ValueError("give exactly one source: --mesh X.ply [--pc2 M.pc2], --glb X.glb or --smpl SMPL.npz --poses X.npy")
    if pc2 is not None and mesh is None:
        raise ValueError("--pc2 needs the --mesh it was written for")
    if (eye is None) != (at is None):
        raise ValueError("--eye and --at go together: where the camera stands and what it looks at")
    if eye is not None and focus is not None:
        raise ValueError("--focus frames the camera itself: it does not go with --eye / --at")
    if focus is not None:
        focus = parse_focus(focus) if isinstance(focus, str) else tuple(focus)
    clip = bool(clip) or focus is not None or eye is not None
    check_raster(size, ss)
    if os.path.splitext(out)[1].lower() not in (".gif", ".png"):
        raise ValueError("--out ends in .gif or .png, got %r" % out)
    if up is None:
        up = "z" if pc2 is not None else "y"
    texture = None
    if mesh is not None:
        v, t, c, moving = mesh_source(mesh, pc2, every)
    elif glb is not None:
        v, t, c, moving, texture = glb_source(glb, every, return_texture=True)
        if texture is not None and clip:
            raise ValueError("a .glb with a baked texture has no clipped preview yet: leave out --clip, --focus and --eye / --at")
    else:
        v, t, c, moving = smpl_source(smpl, poses, every)
    v = v if torch.is_tensor(v) else torch.from_numpy(v).cuda()
    T = v.shape[0]
    n = T if moving else int(views)
    if eye is not None:
        eyes, ats = np.asarray(eye, np.float64).reshape(1, 3), np.asarray(at, np.float64).reshape(1, 3)
        near = far = None                                     # render_frames' default: the whole mesh's range seen from the eye
    else:
        eyes, ats, near, far = frame_cameras(v, n if (orbit or not moving) else 1, elevation, up, fov, margin, focus=focus)
    images = render_frames(v, t, None if texture is not None else c, eyes, ats, up=up, fov=fov, image_size=size, ss=ss, near=near, far=far, clip=clip,
                           texture=texture)
    return save_frames(images, out, fps, frames_dir), images


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", default=None, help="a .ply (Runner.validate_mesh's, or drive's <name>_cleaned_apose.ply)")
    ap.add_argument("--pc2", default=None, help="drive's point cache of that mesh: plays its frames")
    ap.add_argument("--glb", default=None, help="rig's .glb: plays its rotation tracks, or shows the rest pose")
    ap.add_argument("--smpl", default=None, help="the SMPL model (.npz export or the official .pkl): the body itself, in the poses of --poses")
    ap.add_argument("--poses", default=None, help="animate's candidate_<i>.npy (one pose: a turn-table) or motion.npy (played), for --smpl")
    ap.add_argument("--out", required=True, help="P.gif (all frames) or P.png (the first)")
    ap.add_argument("--views", type=int, default=36, help="frames of the turn-table of a static source")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ss", type=int, default=2, help="supersampling, 1 or 2 (size * ss <= %d)" % MAX_RASTER)
    ap.add_argument("--up", choices=("y", "z"), default=None, help="the file's up axis (default: y; z with --pc2, drive writes Blender's frame)")
    ap.add_argument("--elevation", type=float, default=10.0, help="degrees the camera stands above the horizon")
    ap.add_argument("--fov", type=float, default=40.0, help="full field of view in degrees")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--every", type=int, default=1, help="take every k-th frame of a motion")
    ap.add_argument("--frames-dir", default=None, help="also write every frame as a numbered PNG there")
    ap.add_argument("--orbit", action="store_true", help="a moving source: the camera goes round once while the motion plays")
    ap.add_argument("--focus", default=None, help="a close-up of a band of the mesh's height: head (0.84:1), upper (0.5:1), lower (0:0.5) or LO:HI")
    ap.add_argument("--eye", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="a hand-placed fixed camera: where it stands (with --at)")
    ap.add_argument("--at", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="... and the point it looks at")
    ap.add_argument("--clip", action="store_true", help="clip faces at the frustum instead of dropping them (implied by --focus and --eye)")
    args = ap.parse_args(argv)
    try:
        if args.views < 1 or args.every < 1 or args.fps <= 0:
            raise ValueError("--views, --every and --fps are positive")
        out, _ = preview(args.out, mesh=args.mesh, pc2=args.pc2, glb=args.glb, views=args.views, size=args.size, ss=args.ss, up=args.up,
                         elevation=args.elevation, fov=args.fov, fps=args.fps, every=args.every, frames_dir=args.frames_dir, orbit=args.orbit,
                         smpl=args.smpl, poses=args.poses, focus=args.focus, eye=args.eye, at=args.at, clip=args.clip)
    except ValueError as e:
        raise SystemExit("preview: %s" % e)
    print(out)


if __name__ == "__main__":
    main()
