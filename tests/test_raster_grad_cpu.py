"""The rules of neural_renderer's approximate rasteriser backward (tests/nr_grad_restatement.py) on hand-built cases and,
restated in float64, against the geometry of random triangles; the torch side of avatarclip_amd.mesh_render (light from the vertices, projection
Jacobian, vertex -> face CSR), and the CLIP-guided generators of avatarclip_amd.animate with AnimateContext(renderer_gradient=True) on CPU
stand-ins."""
import numpy as np
import pytest
import torch

from tests import nr_grad_restatement as R

N_PIX = 16
EPS = 1e-4
LIGHT = 0.75
# pixel coordinates of a front-facing triangle on a 16 x 16 super-sampled grid: edge 0 (v0 -> v1) is the vertical line x = 10.3
P = np.array([[10.3, 2.2], [10.3, 12.2], [3.3, 7.2]])


def _triangle(P=P):
    ndc = np.zeros((3, 3), np.float32)
    ndc[:, :2] = (2 * P - (N_PIX - 1)) / N_PIX            # P = 0.5 (ndc n + n - 1)
    ndc[:, 2] = 2.0
    faces = np.array([[0, 1, 2]])
    return ndc, faces, R.rasterize_index(ndc, faces, N_PIX)


def _one_hot(x, y, g):
    G = np.zeros((N_PIX, N_PIX), np.float32)
    G[y, x] = g
    return G


def _push(d):
    return d + EPS if d > 0 else d - EPS


def test_the_triangle_covers_what_its_edges_say():
    ndc, faces, fi = _triangle()
    assert not R.is_back(ndc[faces[0]])
    assert fi[6, 10] == 0 and fi[6, 11] == -1 and fi[6, 5] == 0 and fi[6, 4] == -1 and fi[12, 10] == -1


def test_a_pixel_just_outside_an_edge_moves_that_edges_two_vertices():
    """G at (x 12, y 6), right of the vertical edge x = 10.3: only edge 0's out run on scan line y = 6 (axis 1: u = y, w = x, dir +1) reaches it.
    Delta = (c(12) - c(w_in = 10)) G = (0 - L) g > 0 for g < 0; the x components of v0 and v1 move by -Delta / d."""
    ndc, faces, fi = _triangle()
    g = -1.0
    grad = R.pseudo_grad(ndc, faces, [LIGHT], fi, _one_hot(12, 6, g), EPS)
    ua, ub, u0, w, wx = 2.2, 12.2, 6.0, 12.0, 10.3
    delta = (0.0 - LIGHT) * g
    d_a = _push((ub - ua) / (ub - u0) * (w - wx) * 2 / N_PIX)
    d_b = _push((ub - ua) / (u0 - ua) * (w - wx) * 2 / N_PIX)
    expect = np.zeros((3, 3))
    expect[0, 0], expect[1, 0] = -delta / d_a, -delta / d_b
    assert np.allclose(grad, expect, rtol=2e-5, atol=0), (grad, expect)
    # the same pixel with an upstream gradient of the other sign: Delta <= 0, nothing
    assert not R.pseudo_grad(ndc, faces, [LIGHT], fi, _one_hot(12, 6, -g), EPS).any()


def test_a_pixel_just_inside_gets_the_in_runs_of_the_edges_that_cross_its_lines():
    """G at (x 10, y 6), inside, next to edge 0: scan line y = 6 crosses edge 0 (dir +1, w_x = 10.3) and edge 2 (dir -1); column x = 10 crosses
    edge 1 (dir +1) and edge 2 (dir -1).  Every in run holding the pixel gives Delta = (L - 0) g > 0; edge 0's term is the one the edge's
    own displacement (w - w_x = -0.3) makes, the others follow the same formula with their own crossings."""
    ndc, faces, fi = _triangle()
    g = 1.0
    grad = R.pseudo_grad(ndc, faces, [LIGHT], fi, _one_hot(10, 6, g), EPS)
    delta = LIGHT * g
    p = R.pixel_coords(ndc, N_PIX).astype(np.float64)
    expect = np.zeros((3, 3))

    def term(a, b, axis, u0, w):
        ua, ub = p[a, 0 if axis == 0 else 1], p[b, 0 if axis == 0 else 1]
        wa, wb = p[a, 1 if axis == 0 else 0], p[b, 1 if axis == 0 else 0]
        wx = (wb - wa) / (ub - ua) * (u0 - ua) + wa
        comp = 1 if axis == 0 else 0
        expect[a, comp] -= delta / _push((ub - ua) / (ub - u0) * (w - wx) * 2 / N_PIX)
        expect[b, comp] -= delta / _push((ub - ua) / (u0 - ua) * (w - wx) * 2 / N_PIX)

    term(0, 1, 1, 6.0, 10.0)       # edge 0 along y = 6: w_x = 10.3, the run from x = 10 to the opposite edge holds x = 10
    term(2, 0, 1, 6.0, 10.0)       # edge 2 along y = 6: w_x = 4.98, the run from x = 5 to edge 0 (x = 10.3 -> 10)
    term(1, 2, 0, 10.0, 6.0)       # edge 1 along x = 10: w_x = 11.99, run down to edge 2 (y = 2.41 -> 3)
    term(2, 0, 0, 10.0, 6.0)       # edge 2 along x = 10: w_x = 2.41, run up to edge 1
    assert np.allclose(grad, expect, rtol=1e-4, atol=1e-6), (grad, expect)
    assert grad[0, 0] > 0 and grad[1, 0] > 0     # a loss that grows with the face's brightness there: descent moves edge 0 to the left (-x)
    assert abs(grad[:, 2]).max() == 0


def test_back_faces_and_zero_gradients_give_nothing():
    ndc, faces, fi = _triangle()
    G = np.random.RandomState(0).randn(N_PIX, N_PIX).astype(np.float32)
    assert not R.pseudo_grad(ndc, faces, [LIGHT], fi, np.zeros_like(G), EPS).any()
    back = faces[:, ::-1].copy()
    assert R.is_back(ndc[back[0]])
    assert not R.pseudo_grad(ndc, back, [LIGHT], fi, G, EPS).any()
    assert (R.rasterize_index(ndc, back, N_PIX) == -1).all()


def test_light_gradient_sums_the_faces_pixels():
    ndc, faces, fi = _triangle()
    G = np.random.RandomState(1).randn(N_PIX, N_PIX).astype(np.float32)
    assert np.isclose(R.light_grad(fi, G, 1)[0], G[fi == 0].astype(np.float64).sum())
    gi = np.random.RandomState(2).randn(N_PIX // 2, N_PIX // 2).astype(np.float32)
    Gm = R.G_map(gi)
    assert Gm[0, 0] == gi[-1, 0] / 4 and Gm[N_PIX - 1, 1] == gi[0, 0] / 4 and Gm[2, 3] == gi[N_PIX // 2 - 2, 1] / 4


def test_light_and_projection_jacobian_gradcheck():
    from avatarclip_amd import mesh_render as M
    rs = np.random.RandomState(0)
    v = torch.from_numpy(rs.uniform(-0.5, 0.5, (8, 3))).double().requires_grad_(True)
    f = torch.from_numpy(np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [1, 6, 7]]))
    assert torch.autograd.gradcheck(lambda x: M.face_light(x, f), (v,))
    cams = np.stack([M.camera_frame(np.array([0.3, 0.2, 2.0], np.float32), np.array([-0.1, -0.1, -1.0], np.float32)),
                     M.camera_frame(np.array([0.0, 0.1, 0.3], np.float32), np.array([0.0, 0.0, -1.0], np.float32))])
    cam = torch.from_numpy(cams).double()
    vv = torch.from_numpy(rs.uniform(-0.5, 0.5, (2, 8, 3))).double().requires_grad_(True)
    width = float(np.tan(np.deg2rad(30.0)))
    assert torch.autograd.gradcheck(lambda x: M.project(x, cam, width), (vv,))
    g = torch.from_numpy(rs.randn(2, 8, 3))
    ref, = torch.autograd.grad((M.project(vv, cam, width) * g).sum(), vv)
    mine = M.project_vjp(vv.detach(), cam, width, g)
    assert torch.allclose(mine, ref, atol=1e-12)
    behind = (torch.einsum("nvk,njk->nvj", vv.detach() - cam[:, None, :3], cam[:, 3:].reshape(-1, 3, 3))[..., 2] <= 0)
    assert behind.any() and (mine[behind] == 0).all()           # the reference README's patch: no gradient behind the camera


def test_vertex_face_csr():
    from avatarclip_amd import mesh_render as M
    f2 = np.array([[0, 1, 2], [2, 1, 3], [2, 1, 0], [3, 1, 2]])
    ptr, ent = M.vertex_face_csr(f2, 5)
    assert ptr.tolist() == [0, 2, 6, 10, 12, 12]
    for v in range(5):
        got = ent[ptr[v]:ptr[v + 1]]
        assert all(f2[e // 3, e % 3] == v for e in got) and list(got) == sorted(got)
    with pytest.raises(ValueError):
        M.vertex_face_csr(f2, 3)


def _runs(P, fi, n):
    """DESIGN.md section 8's visits for face 0 of pixel-space vertices P [3,2], restated in float64 (not the restatement's arithmetic) ->
    (a, b, o, axis, u0, w_x, w, is the in run's pixel at w_in) for every run pixel"""
    out = []
    for e in range(3):
        a, b, o = e, (e + 1) % 3, (e + 2) % 3
        for axis in (0, 1):
            ui, wi = (0, 1) if axis == 0 else (1, 0)
            ua, wa, ub, wb, uo, wo = P[a, ui], P[a, wi], P[b, ui], P[b, wi], P[o, ui], P[o, wi]
            d = (-1 if ua < ub else 1) if axis == 0 else (1 if ua < ub else -1)
            at = (lambda u, w: (w, u)) if axis == 0 else (lambda u, w: (u, w))
            for u0 in range(max(int(np.ceil(min(ua, ub))), 0), int(min(max(ua, ub), n - 1)) + 1):
                wx = (wb - wa) / (ub - ua) * (u0 - ua) + wa
                w_in = int(np.floor(wx) if d > 0 else np.ceil(wx))
                w_out = w_in + d
                if not (0 <= w_in < n and 0 <= w_out < n):
                    continue
                if fi[at(u0, w_in)] == 0:
                    out += [(a, b, o, axis, u0, wx, w, False) for w in range(w_out, n if d > 0 else -1, d)]
                wx2 = (wo - wa) / (uo - ua) * (u0 - ua) + wa if (u0 - ua) * (u0 - uo) < 0 else (wb - wo) / (ub - uo) * (u0 - uo) + wo
                lim = int(np.ceil(wx2) if d > 0 else np.floor(wx2))
                out += [(a, b, o, axis, u0, wx, w, w == w_in) for w in range(max(min(w_in, lim), 0), min(max(w_in, lim), n - 1) + 1)
                        if fi[at(u0, w)] == 0]
    return out


def _edge_margin(T, k, x, y):
    """signed distance in pixels of pixel centre (x, y) inside edge k (T[k] -> T[k + 1]) of the counter-clockwise triangle T [3,2]"""
    p, q = T[k], T[(k + 1) % 3]
    return ((q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])) / np.hypot(*(q - p))


def test_the_displacement_rule_moves_the_edge_through_the_pixel():
    """For every run pixel the rules visit on random front-facing triangles: moving vertex a (or b) along w by the rule's d (eps = 0, float64)
    puts the line through it and the other vertex on the pixel centre of scan line u0.  For the in run's first pixel (at w_in), re-rasterising
    (fp32) after 1.01 d drops the pixel from the face and after 0.99 d keeps it -- skipped where the pixel lies within one pixel of the other two
    edges before or after the move (moving a vertex moves its other edge too) or where d = 0."""
    n = 32
    rs = np.random.RandomState(7)
    lines = flips = 0
    for _ in range(10):
        while True:
            ndc = np.zeros((3, 3), np.float32)
            ndc[:, :2] = rs.uniform(-0.85, 0.85, (3, 2))
            ndc[:, 2] = 2.0
            if R.is_back(ndc):
                ndc = ndc[[0, 2, 1]]
            P = 0.5 * (ndc[:, :2].astype(np.float64) * n + n - 1)
            area = 0.5 * ((P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[1, 1] - P[0, 1]) * (P[2, 0] - P[0, 0]))
            if area > 40:
                break
        faces = np.array([[0, 1, 2]])
        fi = R.rasterize_index(ndc, faces, n)
        for a, b, o, axis, u0, wx, w, first in _runs(P, fi, n):
            ui, wi = (0, 1) if axis == 0 else (1, 0)
            ua, wa, ub, wb = P[a, ui], P[a, wi], P[b, ui], P[b, wi]
            dw = w - wx
            if dw == 0:
                continue
            for vert, fixed, guard, d in ((a, b, ub != u0, (ub - ua) / (ub - u0) * dw * 2 / n), (b, a, ua != u0, (ub - ua) / (u0 - ua) * dw * 2 / n)):
                if not guard:
                    continue
                Q = P.copy()
                Q[vert, wi] += d * n / 2                               # d is in NDC: n / 2 pixels per unit
                (uv, wv), (uf, wf) = (Q[vert, ui], Q[vert, wi]), (Q[fixed, ui], Q[fixed, wi])
                cross = wv + (wf - wv) * (u0 - uv) / (uf - uv)
                assert abs(cross - w) <= 1e-9 * max(1.0, abs(w)), (a, b, axis, u0, w, cross)
                lines += 1
                if not first:
                    continue
                x, y = (u0, w) if axis == 0 else (w, u0)
                Q11 = P.copy()
                Q11[vert, wi] += 1.01 * d * n / 2
                if not all(_edge_margin(T, k, x, y) >= 1.0 for T in (P, Q11) for k in (b, o)):      # edge a -> b is edge a
                    continue
                for factor, kept in ((1.01, False), (0.99, True)):
                    moved = ndc.copy()
                    moved[vert, 1 - axis] = np.float32(ndc[vert, 1 - axis].astype(np.float64) + factor * d)
                    assert (R.rasterize_index(moved, faces, n)[y, x] == 0) == kept, (a, b, axis, u0, w, vert, factor, d)
                flips += 1
    print("line crossings checked", lines, "in-run pixels re-rasterised", flips)
    assert lines > 2000 and flips > 100
