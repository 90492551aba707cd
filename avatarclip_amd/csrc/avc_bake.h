/* avc_bake.h -- the texture bake's entry points (csrc/avc_bake.hip) and the preview's textured shade (csrc/avc_preview.hip, beside the
 * shade it shares its body with), a fifth part of the C ABI of include/avc.h.
 *
 * Same conventions as include/avc.h: every pointer is a DEVICE pointer, buffers are caller-allocated, `stream` is a hipStream_t, the calls
 * enqueue and return without synchronising, 0 = ok, otherwise avc_last_error() describes the failure.  The interface revision is that header's
 * AVC_ABI_VERSION (4; avc_version() reports it): added entry points do not change it.  avatarclip_amd/lib.py parses this header last
 * (later_headers(), after headers() and added_headers()) and binds the union of the prototypes.
 *
 * THE CLOSEST POINT OF A TRIANGLE (Ericson, Real-Time Collision Detection, 5.1.5), fp64, the float32 corners widened exactly, one correctly
 * rounded IEEE operation each in the order written, no fused multiply-add.  dot(x, y) = (x0 y0 + x1 y1) + x2 y2.
 *   ab = b - a, ac = c - a, ap = p - a;  d1 = dot(ab, ap), d2 = dot(ac, ap);         d1 <= 0 and d2 <= 0:             (1, 0, 0)
 *   bp = p - b;  d3 = dot(ab, bp), d4 = dot(ac, bp);                                   d3 >= 0 and d4 <= d3:            (0, 1, 0)
 *   vc = d1 d4 - d3 d2;             vc <= 0 and d1 >= 0 and d3 <= 0:   v = d1 / (d1 - d3)                              (1 - v, v, 0)
 *   cp = p - c;  d5 = dot(ab, cp), d6 = dot(ac, cp);                                   d6 >= 0 and d5 <= d6:            (0, 0, 1)
 *   vb = d5 d2 - d1 d6;             vb <= 0 and d2 >= 0 and d6 <= 0:   w = d2 / (d2 - d6)                              (1 - w, 0, w)
 *   va = d3 d6 - d5 d4;   va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:   w = (d4 - d3) / ((d4 - d3) + (d5 - d6))         (0, 1 - w, w)
 *   otherwise   g = 1 / ((va + vb) + vc),  v = vb g,  w = vc g                                                         ((1 - v) - w, v, w)
 * the first rule that holds gives the barycentrics (b0, b1, b2); then q_k = (b0 a_k + b1 b_k) + b2 c_k, e = p - q, dist2 = dot(e, e).
 * A triangle is DEGENERATE when a corner index lies outside [0, V) or every component of ab x ac (n0 = ab1 ac2 - ab2 ac1, n1 = ab2 ac0 -
 * ab0 ac2, n2 = ab0 ac1 - ab1 ac0) is exactly zero; it is never a candidate.  Among candidates the smaller dist2 wins, equal dist2 the lower
 * triangle index.
 *
 * THE GRID.  Cell (x, y, z), 0 <= x < nx ..., has the index (z ny + y) nx + x; a triangle lives in the cell of its centroid
 * g = ((a + b) + c) / 3:  x = min(max(floor((g_x - origin_x) / cell), 0), nx - 1).  The caller guarantees that the box [origin, origin + n cell]
 * holds every centroid and that r_max is at least the largest centroid-to-corner distance (it adds its own slack for the roundings).
 */
#ifndef AVC_BAKE_H
#define AVC_BAKE_H
#ifdef __cplusplus
extern "C" {
#endif

/* keys[f] = (cell index << 32) | f, a degenerate triangle under cell index nx ny nz; r2[f] = the largest squared centroid-to-corner distance
 * (0 for a degenerate one).  v [V,3], t [F,3].  nx, ny, nz in [1, 256]. */
int avc_bake_tri_keys(const float* v, int V, const int* t, int F, double origin_x, double origin_y, double origin_z, double cell, int nx, int ny,
                      int nz, long long* keys, double* r2, void* stream);
/* keys SORTED ascending -> starts [ncells + 1]: starts[c] = the first position whose cell index is >= c (ncells = nx ny nz: starts[ncells] is
 * the number of triangles that are not degenerate).  One lane per position fills the cells between its predecessor's and its own. */
int avc_bake_cell_starts(const long long* keys, int F, int ncells, int* starts, void* stream);
/* The exact closest point of the triangle soup for Q fp64 points [Q,3]: tri [Q] (-1: no candidate at all), bary [Q,3], dist2 [Q].  keys sorted,
 * starts from avc_bake_cell_starts.  One query per lane; the lane walks the shells of growing Chebyshev radius k around the cell of the query
 * clamped into the box, and stops before shell k >= 1 once lb = sqrt(o2 + ((k - 1) cell)^2) - r_max is positive and lb^2 > the best dist2 (o2 =
 * the squared distance from the query to the box), or after the last shell that meets the grid.  visited (may be NULL): the number of
 * candidate triangles each query tested. */
int avc_bake_query(const double* points, int Q, const float* v, int V, const int* t, int F, const long long* keys, const int* starts,
                   double origin_x, double origin_y, double origin_z, double cell, int nx, int ny, int nz, double r_max, int* tri, double* bary,
                   double* dist2, int* visited, void* stream);
/* The atlas of bake.atlas_layout: G x G cells of P x P texels, texel (i, j) = column i, row j FROM THE TOP of a size x size image; inside cell
 * c = (j / P) G + i / P the local index is a = i mod P, b = P - 1 - j mod P (b points UP).  a + b <= P - 1: triangle 2 c, corners (1, 1),
 * (P - 3, 1), (1, P - 3), b1 = (a - 1) / (P - 4), b2 = (b - 1) / (P - 4); otherwise triangle 2 c + 1, corners (P - 2, P - 2), (3, P - 2),
 * (P - 2, 3), b1 = (P - 2 - a) / (P - 5), b2 = (P - 2 - b) / (P - 5); b0 = (1 - b1) - b2 (fp64; a gutter texel extrapolates).
 * texels [Q]: linear indices j size + i of texels whose triangle is below SF.  points[q] = (b0 v0 + b1 v1) + b2 v2 on triangle st of sv. */
int avc_bake_texel_points(const int* texels, int Q, int size, int P, int G, const float* sv, int SV, const int* st, int SF, double* points,
                          void* stream);
/* image[texels[q]] = rint((b0 c0 + b1 c1) + b2 c2) per channel (fp64, half-even, clamped to [0, 255]) with the colours (csize 3 or 4 bytes per
 * vertex, the first three used) of the corners of dense triangle tri[q]; tri[q] outside [0, F) leaves the texel alone.  image [size, size, 3]. */
int avc_bake_colors(const int* texels, int Q, int size, const int* tri, const double* bary, const int* t, int F, const unsigned char* colors,
                    int csize, int V, unsigned char* image, void* stream);

/* avc_preview_shade (include/avc.h) with the colour taken from a texture: uv [V,2] float32 per VERTEX (glTF's convention: v down from the top
 * row), texels uint8 [T,T,3].  With the perspective-correct weights l_i of that call: u = ((l0 u0 + l1 u1) + l2 u2) / den, v likewise;
 * x = u T - 0.5, y = v T - 0.5; x0 = floor(x), fx = x - x0, y0, fy likewise; the four texel indices x0, x0 + 1, y0, y0 + 1 are clamped to
 * [0, T - 1]; per channel top = c(x0, y0) (1 - fx) + c(x0 + 1, y0) fx, bottom = c(x0, y0 + 1) (1 - fx) + c(x0 + 1, y0 + 1) fx, colour =
 * top (1 - fy) + bottom fy; all fp32, one rounded operation each.  Lighting, supersampling, scratch and face_ids are avc_preview_shade's. */
int avc_preview_shade_tex(const int* proj, const float* v, int N, int V, const int* tris, int F, const float* uv, const unsigned char* texels,
                          int T, const float* lights, float ambient, float bg_r, float bg_g, float bg_b, int S, int ss, void* scratch,
                          unsigned char* image, int* face_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif
