"""The SMPL silhouette / colour prior of AppearanceGen (main.py:290-335 `init_smpl`, :360 `render_one_batch`; SURVEY.md
section 8 row f-1) on the device: a posed body mesh rendered from the iteration's camera by the HIP rasteriser
(csrc/avc_raster.hip) with neural_renderer's conventions -- white texture, ambient 0.5 + directional 0.5 face lighting from
(0,1,0), 60 degree field of view, 2x super-sampling, vertices @ rot_mat, output mirrored in x (models/utils.py:108-125).
Nothing leaves the GPU: the reference renders with neural_renderer, copies the image to the host and back every iteration.

The mesh is an input: a posed .obj (`MeshPrior.from_obj`), vertices/faces tensors, or the SMPL arrays + pose
(`MeshPrior.from_smpl`, linear blend skinning in smpl_lbs.py).  No CPU fallback: the rasteriser is a HIP kernel."""
import numpy as np
import torch

from . import lib as L
from . import h2d

ROT_MAT = ((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))    # models/utils.py:114-118

_scratch = {}               # (device, stream, (N, F, S), bytes) -> 0xFF-filled z-buffer scratch of the rasteriser (every call leaves it so)


def camera_frame(eye, direction):
    """neural_renderer/look.py's camera frame, in float32 like there -- on the host (a dozen small launches otherwise) -> [12]: eye, x, y, z axes"""
    f = np.float32
    z = np.asarray(direction, f)
    z = z / f(np.sqrt((z * z).sum(dtype=f)))
    x = np.cross(np.array([0.0, 1.0, 0.0], f), z).astype(f)
    x = x / f(np.sqrt((x * x).sum(dtype=f)))
    y = np.cross(z, x).astype(f)
    y = y / f(np.sqrt((y * y).sum(dtype=f)))
    return np.concatenate([np.asarray(eye, f), x, y, z])


def face_light(v, faces, light_ambient=0.5, light_directional=0.5, light_direction=(0.0, 1.0, 0.0)):
    """neural_renderer/lighting.py in world space (view independent) for one vertex set [V,3] -> light of the fill_back face list [2F]: the
    faces, then their reversed copies; differentiable"""
    fv = v[faces]
    n = torch.cross(fv[:, 0] - fv[:, 1], fv[:, 2] - fv[:, 1], dim=1)
    n = n / n.norm(dim=1, keepdim=True).clamp(min=1e-5)
    c = n @ torch.tensor(light_direction, dtype=v.dtype, device=v.device)
    return torch.cat([light_ambient + light_directional * c.clamp(min=0), light_ambient + light_directional * (-c).clamp(min=0)])


def _scratch_for(device, layout, need):
    """The rasteriser's persistent scratch for one (N, F, S) layout (N z-buffers of 64-bit (depth, face) keys + N large-face lists): all bits
    set = empty, and every successful call LEAVES the z-buffers and the list counts that way (the resolve launch restores what it read), which
    is what saves a 2-MB fill per view.  The list entries (face indices) stay: a buffer is only ever reused for the same layout, where those
    bytes are list entries again.  One buffer per device and HIP stream -- the launches of one render are ordered by their stream, two streams
    must not interleave on one z-buffer (side-stream view preparation, main-stream validation renders)."""
    key = (str(device), L.stream(), layout, need)
    z = _scratch.get(key)
    if z is None:
        for k in [k for k in _scratch if k[:2] == key[:2]]:
            del _scratch[k]
        z = _scratch[key] = torch.full((need,), 255, dtype=torch.uint8, device=device)
    return z


def _checked(name, *args):
    """L.call; when a launch of the sequence reports an error every scratch is dropped (and refilled on its next use), so that stale keys of
    an interrupted render cannot leak into later priors and silhouette masks"""
    try:
        L.call(name, *args)
    except Exception:
        _scratch.clear()
        raise


def read_obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in t[1:4]])
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


class MeshPrior:
    """prior_renderer(eye, at) -> [image_size, image_size, 3] float32 on `device` (0 = background)"""

    def __init__(self, vertices, faces, device="cuda", image_size=256, viewing_angle=30.0, near=0.1, far=100.0,
                 apply_rot_mat=True, light_ambient=0.5, light_directional=0.5, light_direction=(0.0, 1.0, 0.0)):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("MeshPrior rasterises on the MI355X (no CPU fallback)")
        self.device, self.image_size, self.near, self.far = dev, int(image_size), float(near), float(far)
        self.width = float(np.tan(np.deg2rad(viewing_angle)))
        v = torch.as_tensor(np.asarray(vertices, np.float32)).to(dev).reshape(-1, 3)
        if apply_rot_mat:
            v = v @ torch.tensor(ROT_MAT, dtype=torch.float32, device=dev)
        f = torch.as_tensor(np.asarray(faces).astype(np.int64)).to(dev).reshape(-1, 3)
        self.v_world = v.contiguous()
        self.faces2 = torch.cat([f, f.flip(1)], 0)                 # fill_back=True: every face also in reversed order
        self.light2 = face_light(v, f, light_ambient, light_directional, light_direction).contiguous()
        self.lib = L.load()
        self._faces2_i32 = self.faces2.to(torch.int32).contiguous()
        self._ndc = torch.empty_like(self.v_world)

    @classmethod
    def from_obj(cls, path, **kw):
        v, f = read_obj(path)
        return cls(v, f, **kw)

    @classmethod
    def from_smpl(cls, smpl, pose_axis_angle, v_shaped=None, **kw):
        """main.py:296-333: pose [1,24,3] axis-angle (stand_pose.npy, or the T pose with the root turned by pi/2 about x);
        v_shaped = the ShapeGen template (dataset.template_obj) or the SMPL template."""
        from . import smpl_lbs
        dev = smpl["v_template"].device
        pose = torch.as_tensor(np.asarray(pose_axis_angle, np.float32)).to(dev).reshape(-1, 3)
        rot = smpl_lbs.batch_rodrigues(pose).reshape(1, -1, 3, 3)
        vs = smpl["v_template"].reshape(1, -1, 3) if v_shaped is None else torch.as_tensor(np.asarray(v_shaped, np.float32)).to(dev).reshape(1, -1, 3)
        verts, _ = smpl_lbs.lbs(vs, rot, smpl["posedirs"], smpl["J_regressor"], smpl["parents"], smpl["lbs_weights"])
        return cls(verts[0].detach().cpu().numpy(), smpl["faces"], **kw)

    @torch.no_grad()
    def render_grey(self, eye, direction, rgb_flipped=False):
        """nr.Renderer(camera_mode='look')(vertices, faces, ones) -> [S,S] grey image (before the x flip); rgb_flipped: [S,S,3], x-flipped.
        Projection + rasteriser + 2 x 2 average (+ x flip + channels) in four launches (csrc/avc_raster.hip), one upload (the camera)"""
        dev, S, F2 = self.v_world.device, self.image_size, self.faces2.shape[0]
        cam = h2d.upload(camera_frame(eye, direction), dev)
        out = torch.empty((S, S, 3) if rgb_flipped else (S, S), device=dev, dtype=torch.float32)
        zbuf = _scratch_for(dev, (1, F2, S), self.lib.avc_rasterize_scratch_bytes(F2, 2 * S))
        _checked("avc_rasterize_mesh", self.v_world, self.v_world.shape[0], self._faces2_i32, F2, cam, self.width, self.light2, S, self.near,
                 self.far, self._ndc, out, int(rgb_flipped), 3 if rgb_flipped else 1, zbuf)
        return out

    def __call__(self, eye, at):
        eye, at = np.asarray(eye, np.float64), np.asarray(at, np.float64)
        # models/utils.py:124 (`[:, ::-1]`), white texture: R = G = B
        return self.render_grey(eye, (at - eye) / np.linalg.norm(at - eye), rgb_flipped=True)
