"""Differentiable renders of a mesh for AvatarAnimate's CLIP-guided optimisers (AvatarAnimate/models/render.py:10-39):
N grey renders of N vertex sets of one topology in one call, with autograd to the vertices -- and, opt-in, the same renders of the textured
body (render_rgb_batch: neural_renderer's texture sampling on `avc_rasterize_mesh_tex_save` / `_tex_grad`, csrc/avc_raster_tex.hip; the cubes
come from texture.load_obj_texture).

Forward: neural_renderer's conventions as `smpl_prior.MeshPrior.render_grey` applies them (vertices @ rot_mat, fill_back, ambient 0.5 +
directional 0.5 face light, 60 degree field of view, 2 x super-sampling) on the HIP rasteriser (`avc_rasterize_mesh_save`,
csrc/avc_raster.hip): the same kernels as MeshPrior's single render, batched.  Backward: neural_renderer's approximate gradient (Kato, Ushiku and
Harada, "Neural 3D Mesh Renderer", CVPR 2018, section 3.3; `avc_rasterize_mesh_grad`, rules in DESIGN.md section 8) to the projected
vertices and to the face light; the projection Jacobian (zero for vertices behind the camera, the reference README's patch) and the light's
dependence on the face normals are torch.  No CPU fallback.

One host path serves both bodies: `_render_batch` holds what comes before the launch (topology, rot_mat -- or not, `apply_rot_mat=False`, for
vertices that are in the renderer's frame already --, face light, k cameras per vertex set, the camera upload) and `_RasterFn` the launches; the
texture cubes are an argument that selects the entry points and adds the unlit colours to the saved state."""
import numpy as np
import torch

from . import h2d
from . import lib as L
from .smpl_prior import ROT_MAT, _checked, _scratch_for, camera_frame, face_light

DEFAULT_EPS = 1e-4          # neural_renderer's DEFAULT_EPS
TEXTURE_EPS = 1e-4          # the sampling clamp ts - 1 - eps (neural_renderer's rasteriser default)
VIEWING_ANGLE, NEAR, FAR = 30.0, 0.1, 100.0

_topologies = {}            # faces bytes -> (faces2 int32 [2F,3], vf_ptr, vf_ent) on a device


def project(v, cam, width):
    """look + perspective in torch (the arithmetic the kernel does, as a differentiable function): v [N,V,3], cam [N,12] -> ndc [N,V,3]"""
    R = cam[:, 3:].reshape(-1, 3, 3)
    c = torch.einsum("nvk,njk->nvj", v - cam[:, None, :3], R)
    front = c[..., 2:3] > 0
    z = torch.where(front, c[..., 2:3], torch.ones_like(c[..., 2:3]))
    ndc = torch.cat([c[..., :2] / z / width, c[..., 2:3]], -1)
    return torch.where(front, ndc, torch.zeros_like(ndc))


def project_vjp(v, cam, width, grad_ndc):
    """the transpose of project's Jacobian applied to grad_ndc [N,V,3] -> [N,V,3]; zero for vertices behind the camera"""
    R = cam[:, 3:].reshape(-1, 3, 3)
    c = torch.einsum("nvk,njk->nvj", v - cam[:, None, :3], R)
    cz = c[..., 2]
    front = cz > 0
    iz = torch.where(front, 1.0 / torch.where(front, cz, torch.ones_like(cz)), torch.zeros_like(cz))
    gx, gy, gz = grad_ndc.unbind(-1)
    dc = torch.stack([gx * iz / width, gy * iz / width,
                      torch.where(front, gz - (gx * c[..., 0] + gy * c[..., 1]) * iz * iz / width, torch.zeros_like(gz))], -1)
    return torch.einsum("nvj,njk->nvk", dc, R)


def vertex_face_csr(faces2, V):
    """vertex -> (3 face + corner) entries of a face list [F,3], in face order: (ptr [V+1], ent) int32"""
    f = np.asarray(faces2, np.int64).reshape(-1)
    if f.size and (f.min() < 0 or f.max() >= V):
        raise ValueError("face indices outside [0, %d)" % V)
    order = np.argsort(f, kind="stable")
    ptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(f, minlength=V), out=ptr[1:])
    return ptr.astype(np.int32), order.astype(np.int32)


def _topology(faces, V, device):
    f = np.ascontiguousarray(np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).astype(np.int64).reshape(-1, 3))
    key = (f.tobytes(), V, str(device))
    t = _topologies.get(key)
    if t is None:
        f2 = np.concatenate([f, f[:, ::-1]], 0)               # fill_back=True: every face also in reversed order
        ptr, ent = vertex_face_csr(f2, V)
        t = _topologies[key] = (torch.from_numpy(f2.astype(np.int32)).to(device), torch.from_numpy(f).to(device),
                                torch.from_numpy(ptr).to(device), torch.from_numpy(ent).to(device))
    return t


class _RasterFn(torch.autograd.Function):
    """N renders with the state the backward needs.  textures None: the grey entry points, -> (image [N,S,S], ndc, face index).  textures
    [F,ts,ts,ts,3]: the textured ones, -> (image [N,S,S,3], ndc, face index, unlit colours of the super-sampled pixels [N,2S,2S,3])."""

    @staticmethod
    def forward(ctx, v_world, light2, cam, faces2, vf_ptr, vf_ent, S, width, eps, textures=None):
        N, V = v_world.shape[:2]
        F2 = faces2.shape[0]
        dev = v_world.device
        tex = textures is not None
        vw, lt = v_world.detach().float().contiguous(), light2.detach().float().contiguous()
        ndc = torch.empty(N, V, 3, device=dev, dtype=torch.float32)
        image = torch.empty((N, S, S, 3) if tex else (N, S, S), device=dev, dtype=torch.float32)
        unlit = (torch.empty(N, 2 * S, 2 * S, 3, device=dev, dtype=torch.float32),) if tex else ()
        fidx = torch.empty(N, 2 * S, 2 * S, device=dev, dtype=torch.int32)
        scratch = _scratch_for(dev, (N, F2, S), N * L.load().avc_rasterize_scratch_bytes(F2, 2 * S))
        cubes = (textures, textures.shape[0], textures.shape[1], TEXTURE_EPS) if tex else ()
        _checked("avc_rasterize_mesh_tex_save" if tex else "avc_rasterize_mesh_save", vw, N, V, faces2, F2, cam, width, lt, *cubes, S, NEAR, FAR,
                 ndc, image, *unlit, fidx, scratch)
        ctx.save_for_backward(vw, lt, cam, faces2, vf_ptr, vf_ent, ndc, fidx, *unlit)
        ctx.S, ctx.width, ctx.eps = S, width, eps
        ctx.mark_non_differentiable(ndc, fidx, *unlit)
        return (image, ndc, fidx) + unlit

    @staticmethod
    def backward(ctx, g_image, *_g_state):
        vw, lt, cam, faces2, vf_ptr, vf_ent, ndc, fidx, *unlit = ctx.saved_tensors
        N, V = vw.shape[:2]
        F2 = faces2.shape[0]
        g = g_image.float().contiguous()
        face_grad = torch.empty(N, F2, 6, device=vw.device, dtype=torch.float32)
        grad_ndc = torch.empty(N, V, 3, device=vw.device, dtype=torch.float32)
        grad_light = torch.empty(N, F2, device=vw.device, dtype=torch.float32)
        L.call("avc_rasterize_mesh_tex_grad" if unlit else "avc_rasterize_mesh_grad", g, ndc, N, V, faces2, F2, lt, *unlit, fidx, ctx.S, ctx.eps,
               vf_ptr, vf_ent, face_grad, grad_ndc, grad_light)
        gv = project_vjp(vw, cam, ctx.width, grad_ndc) if ctx.needs_input_grad[0] else None
        return (gv, grad_light) + (None,) * 8


def _render_batch(v_world, faces, eyes, directions, textures, image_size, eps, apply_rot_mat):
    """what render_grey_batch and render_rgb_batch share, after their refusals that name a device: the camera count, the topology, rot_mat
    (apply_rot_mat False: the vertices are in the renderer's frame already), the face light, k cameras on every vertex set -> _RasterFn's outputs"""
    dev = v_world.device
    B, V = v_world.shape[:2]
    N = len(eyes)
    if B == 0 or N % B or len(directions) != N:
        raise ValueError("k cameras per vertex set: %d vertex sets, %d eyes, %d directions" % (B, N, len(directions)))
    faces2, f, vf_ptr, vf_ent = _topology(faces, V, dev)
    v = v_world.float()
    if apply_rot_mat:
        v = v @ torch.tensor(ROT_MAT, dtype=torch.float32, device=dev)
    light2 = torch.stack([face_light(v[i], f) for i in range(B)])
    if N != B:
        v, light2 = v.repeat(N // B, 1, 1), light2.repeat(N // B, 1)
    cam = h2d.upload(np.stack([camera_frame(e, d) for e, d in zip(eyes, directions)]).reshape(-1), dev).reshape(N, 12)
    width = float(np.tan(np.deg2rad(VIEWING_ANGLE)))
    return _RasterFn.apply(v, light2, cam, faces2, vf_ptr, vf_ent, int(image_size), width, float(eps), textures)


def render_grey_batch(v_world, faces, eyes, directions, image_size=256, eps=DEFAULT_EPS, return_state=False, apply_rot_mat=True):
    """v_world [B,V,3] (before rot_mat; apply_rot_mat False: after it), faces [F,3], eyes / directions: N = k B camera positions / viewing
    directions, render i of vertex set i % B (k cameras, each on all B sets, camera-major; k = 1: one camera per set) -> grey images [N,S,S]
    (row 0 = top, no x flip; 0 = background) with autograd to v_world.  return_state: also (ndc [N,V,3], face index [N,2S,2S] y up)."""
    if v_world.device.type != "cuda":
        raise RuntimeError("render_grey_batch rasterises on the MI355X (no CPU fallback)")
    image, ndc, fidx = _render_batch(v_world, faces, eyes, directions, None, image_size, eps, apply_rot_mat)
    return (image, ndc, fidx) if return_state else image


def check_textures(textures, n_faces):
    """the refusals of render_rgb_batch, before any launch: cubes [F,ts,ts,ts,3] for exactly the mesh's faces, ts >= 2, constants"""
    if not torch.is_tensor(textures) or textures.dim() != 5 or textures.shape[-1] != 3 or len(set(textures.shape[1:4])) != 1:
        raise ValueError("textures are cubes [F,ts,ts,ts,3], got %s" % (list(textures.shape) if torch.is_tensor(textures) else type(textures).__name__))
    if textures.shape[0] != n_faces:
        raise ValueError("textures hold the cubes of %d faces, the mesh has %d faces" % (textures.shape[0], n_faces))
    if textures.shape[1] < 2:
        raise ValueError("texture_size = %d; a texture cube needs at least 2 texels per axis (texel i is blended with i + 1)" % textures.shape[1])
    if textures.requires_grad:
        raise ValueError("the texture cubes are constants of the render: a gradient to them is not implemented, pass textures.detach()")


def render_rgb_batch(v_world, faces, textures, eyes, directions, image_size=256, eps=DEFAULT_EPS, return_state=False, apply_rot_mat=True):
    """render_grey_batch of the textured body: textures [F,ts,ts,ts,3] float32 on the device (texture.load_obj_texture's cubes; constants) ->
    RGB images [N,3,S,S] with autograd to v_world.  return_state: also (ndc [N,V,3], face index [N,2S,2S] y up, unlit colours [N,2S,2S,3] y up)."""
    dev = v_world.device
    check_textures(textures, len(faces))
    if dev.type != "cuda" or textures.device != dev:
        raise RuntimeError("render_rgb_batch rasterises on the MI355X (no CPU fallback): vertices on %s, textures on %s" % (dev, textures.device))
    image, ndc, fidx, unlit = _render_batch(v_world, faces, eyes, directions, textures.float().contiguous(), image_size, eps, apply_rot_mat)
    image = image.permute(0, 3, 1, 2)
    return (image, ndc, fidx, unlit) if return_state else image


def render_batch(v_world, faces, eyes, directions, textures=None, image_size=256, eps=DEFAULT_EPS, apply_rot_mat=True):
    """the body as the CLIP tower takes it, [N,3,S,S]: render_rgb_batch of the cubes, or (textures None) render_grey_batch's white body on
    three channels"""
    if textures is not None:
        return render_rgb_batch(v_world, faces, textures, eyes, directions, image_size, eps, apply_rot_mat=apply_rot_mat)
    return render_grey_batch(v_world, faces, eyes, directions, image_size, eps, apply_rot_mat=apply_rot_mat).unsqueeze(1).expand(-1, 3, -1, -1)
