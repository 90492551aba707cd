/* avc_preview_clip.h -- the clipping entry points of the preview renderer (csrc/avc_preview_clip.hip), a fourth part of the C ABI of
 * include/avc.h.
 *
 * Same conventions as include/avc.h: every pointer is a DEVICE pointer, buffers are caller-allocated, `stream` is a hipStream_t, the calls
 * enqueue and return without synchronising, 0 = ok, otherwise avc_last_error() describes the failure.  The interface revision is that header's
 * AVC_ABI_VERSION (4; avc_version() reports it): added entry points do not change it.  avatarclip_amd/lib.py parses this header after the three
 * of headers() (added_headers()) and binds the union of their prototypes.
 *
 * avc_preview_raster / avc_preview_shade (include/avc.h) DROP a face with an invalid corner.  The two calls below take their place, after the
 * same avc_preview_project and on the same scratch (avc_preview_scratch_bytes(F, R) per frame, all 0xFF on entry and on return), and CLIP such
 * a face at the frustum instead.  v, cams, width, near, far are what avc_preview_project was given.  The rules, all fp64, one correctly rounded
 * operation each in the order written, no fused multiply-add:
 *   - A face whose three corners are valid is drawn exactly as avc_preview_raster draws it (the same key, the same colour).  Every other
 *     face with indices in [0, V) and finite corner coordinates is clipped; a face with a non-finite coordinate is dropped.
 *   - c(v) = (c_x, c_y, c_z) is the projection's camera-space point.  kp = 1 + (65536 + 256) / (128 R), e = kp width, s = e c_z.  Six
 *     planes in this order: near d = c_z - near, far d = far - c_z, left d = s + c_x, right d = s - c_x, bottom d = s + c_y, top d = s - c_y;
 *     inside <=> d >= 0 (NaN: outside).  The side planes lie one raster pixel outside the guard band, so a valid corner is inside all six
 *     and is never replaced by an intersection.
 *   - The polygon starts as the three corners in the order tris stores them; a vertex carries (c_x, c_y, c_z) and its barycentric triple
 *     ((1,0,0), (0,1,0), (0,0,1)).  Per plane, over the edges A -> B cyclically: A inside: emit A; exactly one of A, B inside: emit the
 *     intersection, always from the inside end P to the outside end Q: t = d_P / (d_P - d_Q), u = u_P + t (u_Q - u_P) for the six carried
 *     numbers, then c_z = near (far) exactly for the near (far) plane.  Later planes recompute d from the carried coordinates.  At most 9
 *     vertices (a tenth is not emitted); fewer than 3 left: nothing is drawn.
 *   - A polygon vertex that is a valid original corner keeps its proj entry; every other one is snapped by the projection's formulas with
 *     X, Y clamped to [-65536 - 256, 256 R + 65536 + 256], Z to [0, 2^24 - 1], 1/w = (float)(1 / c_z).
 *   - Fan: sub-triangle j = (p_0, p_j+1, p_j+2), each oriented, zero-area-skipped, filled and depth-interpolated as a face; its key is
 *     (depth << 32 | ORIGINAL face index).  face_ids reports original faces.
 *   - Shading a pixel a clipped face won at depth q: j* = the lowest j whose sub-triangle covers the pixel with depth q; l_i = (float)w_i
 *     iw_i; L_k = (l_0 b_0k + l_1 b_1k) + l_2 b_2k with the carried barycentrics as fp32; colour = ((L_0 c_0 + L_1 c_1) + L_2 c_2) /
 *     ((L_0 + L_1) + L_2) over the original corners' colours; the flat shade is the original face's.
 * No int64 overflow at R <= 2048: coordinates span D = 2^19 + 2^17 + 512 = 655 872, D^2 = 430 168 080 384 < 2^39, the depth sum is
 * <= area2 (2^24 - 1) < 2^63.
 */
#ifndef AVC_PREVIEW_CLIP_H
#define AVC_PREVIEW_CLIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* avc_preview_raster with the clipper: proj [N,V,4] from avc_preview_project(v, N, V, cams, width, near, far, raster_size, ...). */
int avc_preview_raster_clip(const int* proj, const float* v, int N, int V, const float* cams, float width, float near, float far, const int* tris,
                            int F, int raster_size, void* scratch, void* stream);
/* avc_preview_shade with the clipper: the same arguments, plus the cameras and the frustum the keys were made under. */
int avc_preview_shade_clip(const int* proj, const float* v, int N, int V, const float* cams, float width, float near, float far, const int* tris,
                           int F, const unsigned char* colors, int csize, const float* lights, float ambient, float bg_r, float bg_g, float bg_b,
                           float grey, int S, int ss, void* scratch, unsigned char* image, int* face_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif
