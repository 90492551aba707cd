"""Seeded, differentiable CPU stand-ins for what AvatarAnimate's CLIP-guided optimisers call through (TEST INFRASTRUCTURE ONLY), shared by
scripts/gen_golden_animate_clip.py (which binds them to the reference's own methods) and tests/test_animate_clip_cpu.py (which hands them to
avatarclip_amd.animate): a small SMPL-shaped body, a smooth "render" of its vertices that draws the camera elevations from numpy's generator the
way models/render.py does, and a linear image encoder.  Their content is arbitrary; what they pin is the arithmetic AROUND them."""
import math
import types

import numpy as np
import torch

from avatarclip_amd import smpl_lbs

NV, NF, RES = 48, 40, 16


def smpl_arrays(seed=0):
    rs = np.random.RandomState(seed)
    v = rs.uniform(-0.5, 0.5, (NV, 3)).astype(np.float32)
    w = rs.uniform(0, 1, (NV, 24)).astype(np.float32) ** 4
    w /= w.sum(1, keepdims=True)
    jreg = rs.uniform(0, 1, (24, NV)).astype(np.float32)
    jreg /= jreg.sum(1, keepdims=True)
    parents = np.array([-1] + [int(rs.randint(0, i)) for i in range(1, 24)], np.int64)
    faces = np.stack([rs.choice(NV, 3, replace=False) for _ in range(NF)]).astype(np.int32)
    return dict(v_template=torch.from_numpy(v), posedirs=torch.zeros(23 * 9, NV * 3), J_regressor=torch.from_numpy(jreg),
                parents=torch.from_numpy(parents), lbs_weights=torch.from_numpy(w), faces=faces)


class SMPLStandIn:
    """the reference's `self.smpl` (smplx.create(..., 'smpl')): smpl(body_pose=[bs,69], global_orient=[bs,3]).vertices"""

    def __init__(self, arrays):
        self.a, self.faces = arrays, arrays["faces"]

    def __call__(self, body_pose, global_orient):
        bs = body_pose.shape[0]
        full = torch.cat([global_orient.reshape(bs, 1, 3), body_pose.reshape(bs, 23, 3)], dim=1)
        rot = smpl_lbs.batch_rodrigues(full.reshape(-1, 3)).reshape(bs, 24, 3, 3)
        a = self.a
        v, _ = smpl_lbs.lbs(a["v_template"][None].expand(bs, -1, -1), rot, a["posedirs"], a["J_regressor"], a["parents"], a["lbs_weights"])
        return types.SimpleNamespace(vertices=v)


_W = torch.from_numpy(np.random.RandomState(7).randn(RES * RES, 3 * NV).astype(np.float32) * 0.4)


def render(vertices, faces, angles):
    """models/render.py's interface and draw order (np.random.randn() * 0.3 degrees of elevation per angle, before the batch loop): vertices
    [bs,V,3] -> images [len(angles) * bs, 3, RES, RES] in [0,1], camera-major; each image a smooth function of the vertices seen from the camera"""
    elev = [np.random.randn() * 0.3 for _ in angles]
    out = []
    for a, e in zip(angles, elev):
        az, el = math.radians(a), math.radians(e)
        ca, sa, ce, se = math.cos(az), math.sin(az), math.cos(el), math.sin(el)
        R = torch.tensor([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]], dtype=vertices.dtype) @ \
            torch.tensor([[1.0, 0.0, 0.0], [0.0, ce, -se], [0.0, se, ce]], dtype=vertices.dtype)
        v = vertices @ R
        img = torch.sigmoid(v.reshape(v.shape[0], -1) @ _W.t()).reshape(-1, 1, RES, RES)
        out.append(img.expand(-1, 3, -1, -1))
    return torch.cat(out, 0)


def render_one_batch(vertices, faces, angles, device):
    """the same under the reference's name and signature"""
    return render(vertices, faces, angles)


class Perceptor(torch.nn.Module):
    """encode_image([B,3,224,224]) -> [B,512]: 32 x 32 average pooling and a fixed linear map"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("w", torch.randn(3 * 7 * 7, 512, generator=g) * 0.2)
        self.register_buffer("b", torch.randn(512, generator=g))

    def encode_image(self, x):
        return torch.nn.functional.avg_pool2d(x, 32).reshape(x.shape[0], -1) @ self.w + self.b
