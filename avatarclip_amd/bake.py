"""Bake a dense mesh's vertex colours into a texture atlas on a simplified mesh (rig --bake_texture): triangle count and colour resolution
stop being one knob.

    uv, owner = atlas_layout(num_triangles, size)                       the atlas: one chart per triangle, numpy
    tri, bary, d2 = closest_on_mesh(points, vertices, triangles)        the exact closest point of a triangle soup, fp64 (csrc/avc_bake.hip)
    uv, image = bake_texture(simple_v, simple_t, dense_v, dense_t, dense_colors_u8, size)

The atlas (csrc/avc_bake.h): G x G square cells of P x P texels, G = ceil(sqrt(ceil(F / 2))), P = size // G; triangles
2c and 2c + 1 are the lower-left and the upper-right right triangle of cell c (cells row by row from the TOP-left of the image).  With the
cell's local texel index (a, b), a to the right and b UP: chart 2c has its corners at (1, 1), (P - 3, 1), (1, P - 3) and owns a + b <= P - 1;
chart 2c + 1 has them at (P - 2, P - 2), (3, P - 2), (P - 2, 3) and owns a + b >= P.  Corners lie on texel centres; every texel a bilinear
fetch reads anywhere on the closed UV triangle belongs to the chart (a gutter of one texel on every side, baked like any other texel by
extrapolating the chart's affine map); no texel has two owners.  ONE TEXEL DENSITY FOR EVERY CHART whatever the triangle's size or shape:
vertex clustering makes near-uniform triangles, and the packing stays a formula."""
import math
import time

import numpy as np
import torch

from . import drive
from . import lib as L

MIN_SIZE, MAX_SIZE = 64, 4096
MIN_CHART = 6                             # P: the smallest cell in which both charts keep three distinct corners and their gutters
MAX_AXIS = 256                            # BK_MAX_AXIS: grid cells per axis
FREE = 128                                # the mid-grey of a texel no chart owns


def atlas_cells(num_triangles, size):
    """(G, P) of the atlas; ValueError for a bad size or a chart below 6 x 6 texels"""
    F, size = int(num_triangles), int(size)
    if F < 1:
        raise ValueError("atlas_layout: no triangle")
    if size % 4 or not MIN_SIZE <= size <= MAX_SIZE:
        raise ValueError("atlas_layout: size must be a multiple of 4 in [%d, %d], got %d" % (MIN_SIZE, MAX_SIZE, size))
    cells = (F + 1) // 2
    G = math.isqrt(cells - 1) + 1                             # ceil(sqrt(cells)) in integers
    P = size // G
    if P < MIN_CHART:
        need = -(-MIN_CHART * G // 4) * 4
        raise ValueError("atlas_layout: %d triangles need %d x %d cells, %d texels each at size %d; charts need %d: the smallest size that would "
                         "do is %d%s" % (F, G, G, P, size, MIN_CHART, need, "" if need <= MAX_SIZE else " (above the limit of %d: simplify further)" % MAX_SIZE))
    return G, P


def chart_corners(num_triangles, G, P):
    """int64 [F,3,2]: the texel (i, j) = (column, row from the top) of every chart's three corners"""
    f = np.arange(int(num_triangles), dtype=np.int64)
    c, upper = f // 2, (f % 2).astype(bool)
    col, row = c % G, c // G
    lo = np.array([[1, 1], [P - 3, 1], [1, P - 3]], np.int64)
    hi = np.array([[P - 2, P - 2], [3, P - 2], [P - 2, 3]], np.int64)
    ab = np.where(upper[:, None, None], hi[None], lo[None])                         # local (a, b), b up
    return np.stack([col[:, None] * P + ab[:, :, 0], row[:, None] * P + (P - 1 - ab[:, :, 1])], -1)


def atlas_layout(num_triangles, size):
    """uv float32 [F,3,2] (glTF: u = (i + 0.5) / size, v = (j + 0.5) / size for texel column i, row j from the top) and owner int32
    [size, size] (owner[j, i]: the triangle whose chart holds the texel, -1: free)"""
    F, size = int(num_triangles), int(size)
    G, P = atlas_cells(F, size)
    uv = ((chart_corners(F, G, P).astype(np.float64) + 0.5) / float(size)).astype(np.float32)
    i, j = np.arange(size, dtype=np.int64)[None, :], np.arange(size, dtype=np.int64)[:, None]
    col, row = i // P, j // P
    a, b = i % P, P - 1 - j % P
    tri = 2 * (row * G + col) + (a + b > P - 1)
    owner = np.where((col < G) & (row < G) & (tri < F), tri, -1).astype(np.int32)
    return uv, owner


# ---------------------------------------------------------------------------------------------------------------- the closest point
def _mesh_on_device(vertices, triangles, device, what):
    v = (vertices if torch.is_tensor(vertices) else torch.as_tensor(np.asarray(vertices)))
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0:
        raise ValueError("%s: vertices must be [N > 0, 3], got %s" % (what, tuple(v.shape)))
    v = v.to(device=device, dtype=torch.float32).contiguous()
    t = drive._i32(triangles, device).reshape(-1, 3)
    if t.shape[0] == 0:
        raise ValueError("%s: no triangle" % what)
    if int(t.min()) < 0 or int(t.max()) >= v.shape[0]:
        raise ValueError("%s: a triangle names a vertex outside [0, %d)" % (what, v.shape[0]))
    if not bool(torch.isfinite(v).all()):
        raise ValueError("%s: a vertex is not finite" % what)
    return v, t


class Grid:
    """the uniform grid of build_grid: device tensors `keys` (sorted, int64 [F]) and `starts` (int32 [ncells + 1]), `origin` (three Python
    floats), `cell`, `dims` (nx, ny, nz), `r_max` (with its slack), `valid` (the number of triangles that are not degenerate)"""
    __slots__ = ("keys", "starts", "origin", "cell", "dims", "r_max", "valid")


def build_grid(v, t, cell=None):
    """The grid over the triangles t [F,3] int32 of v [V,3] float32 (checked device tensors), binned by centroid cell.  cell: the cell
    size; default twice the median edge length; either is raised until the longest axis has at most 256 cells.  ValueError when every
    triangle is degenerate."""
    F = t.shape[0]
    s = L.stream()
    mn, mx = torch.aminmax(v.double(), dim=0)
    ext = (mx - mn).cpu().numpy()
    origin = [float(x) for x in mn.cpu().numpy()]
    if cell is None:
        tl = t.long()
        e = torch.cat([(v[tl[:, i]] - v[tl[:, (i + 1) % 3]]).double().norm(dim=1) for i in range(3)])
        cell = 2.0 * float(e.median())
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        cell = 1.0
    cell = max(cell, float(ext.max()) / (MAX_AXIS - 1))        # floor(ext / cell) + 1 <= 256
    dims = [min(MAX_AXIS, int(math.floor(float(x) / cell)) + 1) for x in ext]
    ncells = dims[0] * dims[1] * dims[2]
    keys = torch.empty(F, device=v.device, dtype=torch.int64)
    r2 = torch.empty(F, device=v.device, dtype=torch.float64)
    L.call("avc_bake_tri_keys", v, v.shape[0], t, F, origin[0], origin[1], origin[2], cell, dims[0], dims[1], dims[2], keys, r2, stream=s)
    keys = torch.sort(keys).values                             # a cell is a run; its triangles ascend
    starts = torch.empty(ncells + 1, device=v.device, dtype=torch.int32)
    L.call("avc_bake_cell_starts", keys, F, ncells, starts, stream=s)
    g = Grid()
    g.keys, g.starts, g.origin, g.cell, g.dims = keys, starts, origin, cell, dims
    g.valid = int(starts[ncells].item())
    if g.valid == 0:
        raise ValueError("closest_on_mesh: every triangle of the mesh is degenerate")
    # the bound's slack: the roundings of the centroids, of the cell indices and of the squared distances are a few ulps of the extent
    diag = float(np.linalg.norm(ext))
    g.r_max = math.sqrt(float(r2.max())) * (1.0 + 1e-9) + 1e-9 * diag
    return g


def query_grid(points, v, t, grid, count=False):
    """points [Q,3] float64 device tensor -> (tri int32 [Q], bary float64 [Q,3], d2 float64 [Q]) and, with count, the candidates tested per
    query (int32 [Q])"""
    Q = points.shape[0]
    dev = v.device
    tri = torch.empty(Q, device=dev, dtype=torch.int32)
    bary = torch.empty(Q, 3, device=dev, dtype=torch.float64)
    d2 = torch.empty(Q, device=dev, dtype=torch.float64)
    seen = torch.empty(Q, device=dev, dtype=torch.int32) if count else None
    L.call("avc_bake_query", points, Q, v, v.shape[0], t, t.shape[0], grid.keys, grid.starts, grid.origin[0], grid.origin[1], grid.origin[2],
           grid.cell, grid.dims[0], grid.dims[1], grid.dims[2], grid.r_max, tri, bary, d2, seen, stream=L.stream())
    return (tri, bary, d2, seen) if count else (tri, bary, d2)


def closest_on_mesh(points, vertices, triangles, cell=None):
    """The exact closest point of every query on the triangle soup: points [Q,3] (taken as float64), vertices [V,3] float32 (widened
    exactly), triangles [F,3] -- arrays or device tensors.  Returns device tensors (tri int32 [Q], bary float64 [Q,3], d2 float64 [Q]): the
    triangle, the closest point's barycentrics on it and the squared distance, all arithmetic fp64 in the order csrc/avc_bake.h states
    (Ericson 5.1.5).  The smaller d2 wins, equal d2 the lower triangle index; a triangle whose fp64 cross product is exactly zero is
    ignored, and a mesh of such triangles alone is a ValueError.  cell: the grid's cell size (default: twice the median edge length); it
    changes the time, never the result."""
    device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device("cuda")
    v, t = _mesh_on_device(vertices, triangles, device, "closest_on_mesh")
    p = (points if torch.is_tensor(points) else torch.as_tensor(np.asarray(points, np.float64)))
    if p.dim() != 2 or p.shape[1] != 3:
        raise ValueError("closest_on_mesh: points must be [Q, 3], got %s" % (tuple(p.shape),))
    p = p.to(device=device, dtype=torch.float64).contiguous()
    if not bool(torch.isfinite(p).all()):
        raise ValueError("closest_on_mesh: a point is not finite")
    return query_grid(p, v, t, build_grid(v, t, cell))


# ---------------------------------------------------------------------------------------------------------------- the bake
def bake_texture(simple_v, simple_t, dense_v, dense_t, dense_colors_u8, size, stats=None):
    """(uv float32 [F',3,2], image uint8 [size,size,3], numpy).  Every texel a chart of atlas_layout(F', size) owns takes its barycentrics
    in the chart (affine: a gutter texel extrapolates), the fp64 point (b0 v0 + b1 v1) + b2 v2 on the simplified triangle, that point's
    closest point on the dense mesh, and there the fp64 barycentric mix of the three dense corner colours, rounded half-even; a free texel
    is 128.  dense_colors_u8 [N,3|4] uint8 (None: ValueError).  stats: a dict that receives the seconds of the grid build, the query and
    the rest, the number of texels and the mean number of candidate triangles per query."""
    if dense_colors_u8 is None:
        raise ValueError("bake_texture: the dense mesh has no colours to bake")
    t0 = time.perf_counter()
    device = dense_v.device if torch.is_tensor(dense_v) and dense_v.is_cuda else torch.device("cuda")
    dv, dt = _mesh_on_device(dense_v, dense_t, device, "bake_texture (dense mesh)")
    sv, st = _mesh_on_device(simple_v, simple_t, device, "bake_texture (simplified mesh)")
    c = torch.as_tensor(np.asarray(dense_colors_u8) if not torch.is_tensor(dense_colors_u8) else dense_colors_u8)
    if c.dim() != 2 or c.shape[0] != dv.shape[0] or c.shape[1] not in (3, 4) or c.dtype != torch.uint8:
        raise ValueError("bake_texture: colours must be [N, 3] or [N, 4] uint8, got %s %s" % (tuple(c.shape), c.dtype))
    c = c.to(device).contiguous()
    size, F = int(size), st.shape[0]
    G, P = atlas_cells(F, size)
    uv, owner = atlas_layout(F, size)
    flat = owner.reshape(-1)
    texels = np.flatnonzero(flat >= 0)
    texels = texels[np.argsort(flat[texels], kind="stable")].astype(np.int32)          # chart by chart: a wavefront's lanes stay together
    Q = texels.shape[0]
    tex_d = torch.from_numpy(texels).to(device)
    s = L.stream()
    points = torch.empty(Q, 3, device=device, dtype=torch.float64)
    L.call("avc_bake_texel_points", tex_d, Q, size, P, G, sv, sv.shape[0], st, F, points, stream=s)
    image = torch.full((size, size, 3), FREE, device=device, dtype=torch.uint8)
    torch.cuda.synchronize(device)
    t1 = time.perf_counter()
    grid = build_grid(dv, dt)
    torch.cuda.synchronize(device)
    t2 = time.perf_counter()
    tri, bary, _, seen = query_grid(points, dv, dt, grid, count=True)
    torch.cuda.synchronize(device)
    t3 = time.perf_counter()
    L.call("avc_bake_colors", tex_d, Q, size, tri, bary, dt, dt.shape[0], c, c.shape[1], dv.shape[0], image, stream=s)
    out = image.cpu().numpy()
    if stats is not None:
        stats.update(texels=Q, chart=P, cells=G, grid_dims=list(grid.dims), grid_cell=grid.cell, grid_seconds=t2 - t1, query_seconds=t3 - t2,
                     rest_seconds=(t1 - t0) + (time.perf_counter() - t3), candidates_per_query=float(seen.double().mean()),
                     candidates_max=int(seen.max()))
    return uv, out
