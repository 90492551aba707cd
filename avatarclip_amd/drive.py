"""Drive the generated avatar with a motion and export a Blender point cache: AvatarGen/AppearanceGen/drive.py (generate_animation :308-376)
on the device.

    python -m avatarclip_amd.drive --mesh X.ply --motion motion.npy --smpl SMPL.npz|pkl --pose_npy stand_pose.npy --out_dir D
                                   [--name General] [--motion_name NAME] [--preview]

writes D/<name>_cleaned_apose.ply (the largest island of the rotated mesh, colours kept) and D/<motion_name>.pc2 (T frames of the re-posed
mesh), the reference's hard-coded paths turned into arguments; with --preview also D/<name>_preview.gif, the motion played by
avatarclip_amd.preview.  The steps and their reference functions:
  rotate (x, y, z) -> (x, -z, y)                        drive.py:317-324
  cleanup_mesh       largest island                      :172-210   csrc/avc_drive.hip (components, island choice, compaction)
  load_template_smpl SMPL template in the stand pose     :223-233   smpl_lbs.lbs (betas = 0, pose blend shapes included)
  find_nearest_ind   nearest template vertex             :235-240   csrc/avc_drive.hip (fp64, bit-identical to np.argmin)
  inv_lbs / lbs      rigid skinning with the nearest template vertex's weights   :242-265   per-template transforms in torch,
                                                                     their application csrc/avc_drive.hip (avc_skin_apply)
  read_pose_my       motion -> rotations, root (pi/2, 0, 0)  :282-293
  write_pc2          POINTCACHE2 header + [T, M, 3] float32  :295-306   streamed in frame chunks
Each mesh vertex takes ONE template vertex's blend weights, so its 4 x 4 transform (and the inverse) is that template vertex's: K = 6890
transforms per frame, not M.  Motion files: [T, 72] as the reference reads them; [T, 69] (what animate.run writes: body pose without the
root) and [T, 63] (padded with 6 zeros, as AvatarAnimate/visualize.py does) are this port's extension, as is a 1-D pose (one frame)."""
import argparse
import os
import struct

import numpy as np
import torch

from . import lib as L
from . import mesh as _mesh
from . import smpl_lbs

# drive.py:318-323: vertices @ R maps (x, y, z) -> (x, -z, y)
ROTATION = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float32)
PC2_START_FRAME, PC2_SAMPLE_RATE = 0.0, 60.0                  # write_pc2's start_frame / sample_rate
PC2_CHUNK_BYTES = 256 << 20                                   # frames per device -> host hand-off of write_pc2's body


def rotate_vertices(vertices):
    """drive.py:317-323 as written: float64 vertices (open3d's) times the float32 rotation, exact; returned as float32"""
    return np.matmul(np.asarray(vertices, np.float32).astype(np.float64), ROTATION).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- islands
def _i32(t, device):
    return torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(device=device, dtype=torch.int32).contiguous()


def mesh_components(triangles, num_vertices, device=None):
    """label[v] = the smallest vertex index of v's connected component in the triangle-edge graph (a vertex in no triangle is an island of
    its own): avc_mesh_components.  int32 device tensor."""
    device = torch.device(device) if device is not None else (triangles.device if torch.is_tensor(triangles) else torch.device("cuda"))
    t = _i32(triangles, device).reshape(-1, 3)
    nv, nf = int(num_vertices), t.shape[0]
    if nf and (int(t.min()) < 0 or int(t.max()) >= nv):
        raise ValueError("a triangle names a vertex outside [0, %d)" % nv)
    label = torch.empty(nv, device=device, dtype=torch.int32)
    L.call("avc_mesh_components", t if nf else None, nf, nv, label)
    return label


def cleanup_mesh(vertices, triangles, colors=None):
    """drive.py:172-210: keep the largest connected island (the most vertices; a tie goes to the island with the smallest vertex index, the
    one the reference's BFS finds first), vertices / colours / triangles in their original order, triangles re-indexed -- what open3d's
    remove_vertices_by_index leaves.  vertices [N,3] float32, triangles [F,3], colors [N,3|4] uint8 or None (device tensors or arrays; the
    device is the vertices' if they are a CUDA tensor, else cuda).  Returns device tensors (vertices, triangles int32, colors uint8 [n,4] or
    None)."""
    device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device("cuda")
    v = vertices if torch.is_tensor(vertices) else torch.as_tensor(np.asarray(vertices))
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError("vertices must be [N, 3], got %s" % (tuple(v.shape),))
    if colors is not None and (colors.ndim != 2 or colors.shape[0] != v.shape[0] or colors.shape[1] not in (3, 4)):
        raise ValueError("colors must be [N, 3] or [N, 4] uint8, got %s" % (tuple(colors.shape),))
    v = v.to(device=device, dtype=torch.float32).contiguous()
    t = _i32(triangles, device).reshape(-1, 3)
    nv, nf = v.shape[0], t.shape[0]
    c = None
    if colors is not None:
        c = torch.as_tensor(np.asarray(colors) if not torch.is_tensor(colors) else colors).to(device=device, dtype=torch.uint8)
        if c.shape[1] == 3:
            c = torch.cat([c, torch.full((nv, 1), 255, device=device, dtype=torch.uint8)], 1)
        c = c.contiguous()
    if nv == 0:
        return v, t, c
    label = mesh_components(t, nv, device)
    count = torch.empty(nv, device=device, dtype=torch.int32)
    best = torch.empty(1, device=device, dtype=torch.int64)
    vflag = torch.empty(nv, device=device, dtype=torch.int32)
    tflag = torch.empty(max(nf, 1), device=device, dtype=torch.int32)
    tp = t if nf else None
    L.call("avc_mesh_largest_island", tp, nf, nv, label, count, best, vflag, tflag)
    vinc = torch.cumsum(vflag, 0, dtype=torch.int32)
    tinc = torch.cumsum(tflag[:nf], 0, dtype=torch.int32)
    n_v, n_t = int(vinc[-1].item()), (int(tinc[-1].item()) if nf else 0)
    vid, tid = vinc - vflag, tinc - tflag[:nf]          # exclusive scans
    v_out = torch.empty(n_v, 3, device=device, dtype=torch.float32)
    t_out = torch.empty(max(n_t, 1), 3, device=device, dtype=torch.int32)
    c_out = torch.empty(n_v, 4, device=device, dtype=torch.uint8) if c is not None else None
    as_words = lambda x: None if x is None else x.view(torch.int32)          # the kernel moves a colour as one 32-bit RGBA word
    L.call("avc_mesh_compact", v, as_words(c), tp, nf, nv, vflag, vid, tflag if nf else None, tid if nf else None, v_out, as_words(c_out),
           t_out if nf else None)
    return v_out, t_out[:n_t], c_out


# ---------------------------------------------------------------------------------------------------------------- template and transforms
def load_template_smpl(smpl_arrays, pose_npy):
    """drive.py:223-233: the SMPL template with betas = 0 in the stand pose (smplx's SMPLLayer forward, pose blend shapes included, through
    smpl_lbs.lbs).  pose_npy: path of stand_pose.npy or its [1, 72] / [72] values.  Returns (vertices [K,3], pose_rot [1,24,3,3]) on the
    arrays' device.  Evaluated on the CPU, as the reference does (one small lbs): the nearest-vertex search downstream is exact, so its
    template should be the reference's to the bit."""
    a = smpl_arrays
    pose = np.load(pose_npy) if isinstance(pose_npy, (str, os.PathLike)) else np.asarray(pose_npy)
    if pose.size != 72:
        raise ValueError("the template pose has 72 values (24 joints x 3), got %d" % pose.size)
    dev = a["v_template"].device
    c = {k: a[k].cpu() for k in ("v_template", "posedirs", "J_regressor", "parents", "lbs_weights")}
    pose_rot = smpl_lbs.batch_rodrigues(torch.from_numpy(np.asarray(pose, np.float32).reshape(-1, 3))).reshape(1, 24, 3, 3)
    verts, _ = smpl_lbs.lbs(c["v_template"][None], pose_rot, c["posedirs"], c["J_regressor"], c["parents"], c["lbs_weights"])
    return verts[0].contiguous().to(dev), pose_rot.to(dev)


def template_transforms(smpl_arrays, rot_mats):
    """T = W A of drive.py:246-248 / :259-261 for every TEMPLATE vertex: rot_mats [B,24,3,3] -> [B, K, 4, 4] (v_shaped = v_template: betas
    = 0, drive.py:224)"""
    a = smpl_arrays
    B = rot_mats.shape[0]
    J = torch.einsum("bik,ji->bjk", a["v_template"][None], a["J_regressor"]).expand(B, -1, -1)
    _, A = smpl_lbs.batch_rigid_transform(rot_mats, J, a["parents"])
    nj = a["J_regressor"].shape[0]
    W = a["lbs_weights"]
    return torch.matmul(W[None].expand(B, -1, -1), A.reshape(B, nj, 16)).reshape(B, W.shape[0], 4, 4)


def rows3(T):
    """[..., 4, 4] -> [..., 12]: rows 0..2, what avc_skin_apply reads"""
    return T[..., :3, :].reshape(T.shape[:-2] + (12,)).contiguous()


def read_pose_my(fname):
    """drive.py:282-293: motion -> rotation matrices [T, 24, 3, 3] (float32, batch_rodrigues with epsilon 1e-8), the root of every frame
    overwritten with (pi/2, 0, 0).  fname: a .npy path or an array.  Accepted layouts: [T, >= 72] (the first 72 columns, as the
    reference), [T, 69] (body pose without the root: animate.run's motion.npy), [T, 63] (padded with 6 zeros, AvatarAnimate/visualize.py);
    a 1-D pose of 63 / 69 / 72+ values is one frame.  The 69 / 63 forms are this port's extension."""
    poses = np.load(fname) if isinstance(fname, (str, os.PathLike)) else np.asarray(fname)
    poses = np.array(poses, dtype=np.float32)        # a copy: the reference overwrites the root in the loaded array
    if poses.ndim == 1:
        poses = poses[None]
    if poses.ndim != 2 or poses.shape[0] == 0 or not (poses.shape[1] in (63, 69) or poses.shape[1] >= 72):
        raise ValueError("a motion is [T, 72], [T, 69] or [T, 63] (or one such pose), got %s" % (poses.shape,))
    if poses.shape[1] == 63:
        poses = np.concatenate([poses, np.zeros((poses.shape[0], 6), np.float32)], 1)
    if poses.shape[1] == 69:
        poses = np.concatenate([np.zeros((poses.shape[0], 3), np.float32), poses], 1)
    poses = np.ascontiguousarray(poses[:, :72])
    poses[:, :3] = 0
    poses[:, 0] = np.pi / 2
    rot = smpl_lbs.batch_rodrigues(torch.from_numpy(poses).reshape(-1, 3))
    return rot.reshape(poses.shape[0], 24, 3, 3)


# ---------------------------------------------------------------------------------------------------------------- kernels
def find_nearest_ind(new_vertices, template_vertices):
    """drive.py:235-240: index of the nearest template vertex of every mesh vertex, bit-identical to the reference's np.argmin over fp64
    distances (avc_nearest_point).  new_vertices [M,3], template_vertices [K,3] float32 device tensors -> int32 [M]."""
    q = new_vertices.to(torch.float32).contiguous()
    r = template_vertices.to(device=q.device, dtype=torch.float32).contiguous()
    M, K = q.shape[0], r.shape[0]
    if q.dim() != 2 or q.shape[1] != 3 or r.dim() != 2 or r.shape[1] != 3:
        raise ValueError("find_nearest_ind takes [M, 3] and [K, 3] points")
    if M and not K:
        raise ValueError("find_nearest_ind: empty template")
    idx = torch.empty(M, device=q.device, dtype=torch.int32)
    if M:
        L.call("avc_nearest_point", q, M, r, K, idx)
    return idx


def skin_apply(xf, idx, points, out=None):
    """out[t, m] = xf[t, idx[m]] (points[m], 1) (avc_skin_apply): xf [T,K,12] (rows3 of the per-template transforms), idx int32 [M],
    points [M,3] -> [T, M, 3].  Every idx must lie in [0, K): checked here (ValueError)."""
    T, K = xf.shape[0], xf.shape[1]
    M = idx.shape[0]
    if xf.dim() != 3 or xf.shape[2] != 12 or points.shape != (M, 3) or idx.dtype != torch.int32:
        raise ValueError("skin_apply takes xf [T,K,12], idx int32 [M], points [M,3]")
    if out is None:
        out = torch.empty(T, M, 3, device=points.device, dtype=torch.float32)
    if M and T:
        if int(idx.min()) < 0 or int(idx.max()) >= K:
            raise ValueError("skin_apply: a template index outside [0, %d)" % K)
        L.call("avc_skin_apply", xf.contiguous(), idx, points.contiguous(), M, K, T, out)
    return out


def inv_lbs(smpl_arrays, vertices, nearest, pose_rot):
    """drive.py:242-253: T-pose vertices = inverse(T) (v, 1) with T the stand-pose transform of each vertex's nearest template vertex"""
    inv = torch.linalg.inv(template_transforms(smpl_arrays, pose_rot))          # [1, K, 4, 4]: K inverses, not M
    return skin_apply(rows3(inv), nearest, vertices)[0]


def lbs(smpl_arrays, tpose_vertices, nearest, rot_mats, out=None):
    """drive.py:255-265 for a batch of frames: rot_mats [T,24,3,3] -> [T, M, 3]"""
    return skin_apply(rows3(template_transforms(smpl_arrays, rot_mats)), nearest, tpose_vertices, out=out)


# ---------------------------------------------------------------------------------------------------------------- point cache
def pc2_header(vcount, num_samples):
    """write_pc2's header (drive.py:297-301)"""
    return struct.pack("<12siiffi", b"POINTCACHE2\0", 1, int(vcount), PC2_START_FRAME, PC2_SAMPLE_RATE, int(num_samples))


def write_pc2(fname, vertices_list, vcount=None, num_samples=None):
    """drive.py:295-306: header + [T, M, 3] little-endian float32.  vertices_list: the reference's list of [M,3] frames, or -- with vcount
    and num_samples given -- an iterable of [n, M, 3] frame chunks, written as they come (host memory bounded by one chunk)."""
    if vcount is None:
        frames = list(vertices_list)
        vcount, num_samples = frames[0].shape[0], len(frames)
        chunks = [np.stack([f.cpu().numpy() if torch.is_tensor(f) else np.asarray(f) for f in frames])]
    else:
        chunks = vertices_list
    written = 0
    with open(fname, "wb") as f:
        f.write(pc2_header(vcount, num_samples))
        for ch in chunks:
            a = ch.cpu().numpy() if torch.is_tensor(ch) else np.asarray(ch)
            a = a.reshape(-1, int(vcount), 3)
            a.astype("<f4").tofile(f)
            written += a.shape[0]
    if written != num_samples:
        raise ValueError("write_pc2: %d frames announced, %d written" % (num_samples, written))
    return fname


def read_pc2(fname):
    """(header fields, frames [T, M, 3]): the inverse of write_pc2 (tests, tools)"""
    with open(fname, "rb") as f:
        head = struct.unpack("<12siiffi", f.read(32))
        frames = np.fromfile(f, dtype="<f4")
    return head, frames.reshape(head[5], head[2], 3)


def posed_frames(smpl_arrays, tpose_vertices, nearest, rot_mats, chunk_bytes=PC2_CHUNK_BYTES):
    """the frames of lbs in chunks of at most chunk_bytes, each handed to the host as it is done"""
    M, T = tpose_vertices.shape[0], rot_mats.shape[0]
    xf = rows3(template_transforms(smpl_arrays, rot_mats))
    n = max(1, min(T, chunk_bytes // max(1, 12 * M)))
    buf = torch.empty(n, M, 3, device=tpose_vertices.device, dtype=torch.float32)
    for t0 in range(0, T, n):
        k = min(n, T - t0)
        skin_apply(xf[t0:t0 + k], nearest, tpose_vertices, out=buf[:k])
        yield buf[:k].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the whole step
def generate_animation(mesh, motion, smpl, pose_npy, out_dir, name="General", motion_name=None, device=None):
    """drive.py:308-376.  mesh: a PLY path (Runner.validate_mesh's) or (vertices, triangles, colors); motion: a .npy path or array; smpl: a
    path (.npz / official .pkl, smpl_lbs.load_smpl_arrays) or the arrays; pose_npy: stand_pose.npy.  Writes out_dir/<name>_cleaned_apose.ply
    and out_dir/<motion_name>.pc2 (motion_name defaults to the motion file's base name, or 'motion'); returns both paths."""
    device = torch.device(device) if device is not None else torch.device("cuda")
    if isinstance(mesh, (str, os.PathLike)):
        v, t, c = _mesh.read_ply(str(mesh))
    else:
        v, t, c = mesh
    if motion_name is None:
        motion_name = os.path.splitext(os.path.basename(motion))[0] if isinstance(motion, (str, os.PathLike)) else "motion"
    rot_mats = read_pose_my(motion).to(device)
    a = smpl_lbs.load_smpl_arrays(smpl, device=str(device)) if isinstance(smpl, (str, os.PathLike)) else \
        {k: (x.to(device) if torch.is_tensor(x) and k != "parents" else x) for k, x in smpl.items()}
    v = torch.from_numpy(rotate_vertices(v)).to(device)
    v, t, c = cleanup_mesh(v, t, c)
    os.makedirs(out_dir, exist_ok=True)
    ply = os.path.join(out_dir, "%s_cleaned_apose.ply" % name)
    _mesh.write_ply(ply, v.cpu().numpy(), t.cpu().numpy(), None if c is None else c.cpu().numpy())
    template, pose_rot = load_template_smpl(a, pose_npy)
    nearest = find_nearest_ind(v, template)
    tpose = inv_lbs(a, v, nearest, pose_rot)
    pc2 = os.path.join(out_dir, "%s.pc2" % motion_name)
    write_pc2(pc2, posed_frames(a, tpose, nearest, rot_mats), vcount=v.shape[0], num_samples=rot_mats.shape[0])
    return ply, pc2


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the avatar's PLY (Runner.validate_mesh)")
    ap.add_argument("--motion", required=True, help="motion .npy: [T,72], [T,69] (animate.run), [T,63] or one pose")
    ap.add_argument("--smpl", required=True, help="SMPL model arrays: .npz or the official .pkl")
    ap.add_argument("--pose_npy", required=True, help="stand_pose.npy: the pose the avatar was generated in")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--name", default="General")
    ap.add_argument("--motion_name", default=None, help="base name of the .pc2 (default: the motion file's)")
    ap.add_argument("--preview", action="store_true", help="also play the .pc2 into <out_dir>/<name>_preview.gif (avatarclip_amd.preview)")
    args = ap.parse_args(argv)
    ply, pc2 = generate_animation(args.mesh, args.motion, args.smpl, args.pose_npy, args.out_dir, name=args.name, motion_name=args.motion_name)
    print(ply)
    print(pc2)
    if args.preview:
        from . import preview
        print(preview.preview(os.path.join(args.out_dir, "%s_preview.gif" % args.name), mesh=ply, pc2=pc2)[0])


if __name__ == "__main__":
    main()
