// Silhouette + flat-shading rasteriser of the SMPL prior and of AvatarAnimate's renders (row f-4): the forward pass of
// `neural_renderer` as AppearanceGen uses it (AvatarGen/AppearanceGen/models/utils.py:108-125, render_one_batch: white
// texture, ambient 0.5 + directional 0.5 face lighting, anti-aliased 256 x 256) -- no host round trip, no neural_renderer.
// Algorithm = the published one of neural_renderer's rasterize_cuda_kernel.cu (restated in oracle/nr_oracle.py, which this
// kernel is tested against): per pixel of the is x is super-sampled grid, nearest front-facing face whose three edge functions
// contain the pixel centre; perspective-correct 1/z from clamped barycentric weights; strict z test (ties -> lower face index).
//
// Index / compare work, no MFMA: F <= ~30k faces x 9 floats, is^2 <= 512^2 pixels, and a face of the posed SMPL body covers a handful
// of pixels.  Face-parallel with a z-buffer of 64-bit keys: one wavefront per face walks the pixels of the face's bounding box (lanes
// = pixels, so a large face is 64-wide too), evaluates the edge functions and the depth exactly as above and does ONE
// atomicMin(zbuf[pixel], depth_bits << 32 | face) per covered pixel -- depths are positive floats (near < z), so the integer order
// of the key is (depth, face index): nearest face, ties to the lower index, independent of the order the atomics arrive in.  A
// second launch turns the keys into the faces' light values and puts the all-ones "empty" key back.  A face whose box holds more than
// RS_LARGE pixels (a close-up, a face cut by the near plane: one wavefront would walk up to the whole image) is only listed; a
// tile-parallel launch in between gives every 16 x 16 pixel tile a scan over that (short) list -- the first version's scheme, which
// is the right one for exactly those faces.  (The first version of this
// file gave every 16 x 16 pixel tile a scan over ALL faces with an LDS survivor list: 0.37 ms for the 27 552 faces of the prior at
// 512^2, bound by the few tiles over the head and the hands where a thousand small faces survive the box test; staging the faces
// through LDS or scanning 1 024 per round did not move that.  profiles/r04_ab_kernels.txt)
//
// Three entry points, one set of kernels: avc_rasterize_mesh_save renders N vertex sets of one topology, each with its own camera, in one call
// (render b = blockIdx.y / .z: its own ndc, z-buffer and large-face list) and saves the face-index map for the backward (avc_raster_grad.hip);
// avc_rasterize_mesh (the prior) is N = 1 of it with the x flip and the three channels; avc_rasterize_faces takes projected faces [F,9], N = 1,
// no projection and no pooling.
#include "avc_common.h"
#include "../../include/avc.h"
#include "avc_raster.h"      // FaceEq, face_setup, face_depth, face_box, load_face, project_vertex, RS_*

#pragma clang fp contract(off)   // same roundings as the fp32 restatement (edge tests are sign tests)

// the projection of project_vertex (avc_raster.h), one thread per vertex of render b = blockIdx.y; cam = device [N,12]
__global__ __launch_bounds__(256) void raster_project_kernel(const float* __restrict__ vw, int V, const float* __restrict__ cam, float width,
                                                         float* __restrict__ ndc) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= V) return;
  project_vertex(vw + (long)b * V * 3, i, cam + 12 * b, width, ndc + (long)b * V * 3);
}
// one wavefront per face of render b = blockIdx.y (its ndc [V,3], z-buffer and large-face list); faces = ndc gathered through idx [F,3], or
// (idx == NULL, one render) ndc = the faces [F,9] themselves: x, y (NDC), z (depth).  `large` = [count - 1 (0xFFFFFFFF = none), face indices ...]
__global__ __launch_bounds__(256) void raster_faces_kernel(const float* __restrict__ ndc, int V, const int* __restrict__ idx, int F, int is,
                                                       float near, float far, unsigned long long* __restrict__ zbufs, unsigned* __restrict__ larges) {
  const int fn = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
  if (fn >= F) return;
  unsigned long long* zbuf = zbufs + (long)b * is * is;
  unsigned* large = larges + (long)b * (F + 2);
  float f[9];
  load_face(ndc + (long)b * V * 3, idx, fn, f);
  FaceEq e;
  if (!face_setup(f, is, e)) return;
  int xa, xb, ya, yb;
  if (!face_box(e, is, xa, xb, ya, yb)) return;
  const int w = xb - xa + 1, h = yb - ya + 1;
  const int n = w * h;
  if (n > RS_LARGE) {
    if (lane == 0) large[1 + (atomicAdd(&large[0], 1u) + 1u)] = (unsigned)fn;
    return;
  }
  for (int k = lane; k < n; k += 64) {
    const int xi = xa + k % w, yi = ya + k / w;
    const float zp = face_depth(e, xi, yi, is, near, far);
    if (zp < 0.f) continue;
    atomicMin(&zbuf[(long)yi * is + xi], ((unsigned long long)__float_as_uint(zp) << 32) | (unsigned)fn);
  }
}
// the listed large faces of render b = blockIdx.z, tile-parallel: thread = pixel of a 16 x 16 tile, every face of the list whose box meets the
// tile is evaluated at the tile's pixels; the running minimum joins the key the small faces left (plain read-modify-write: one thread per pixel)
__global__ __launch_bounds__(256) void raster_large_kernel(const float* __restrict__ ndc, int V, const int* __restrict__ idx, int F, int is, float near,
                                                       float far, unsigned long long* __restrict__ zbufs, const unsigned* __restrict__ larges) {
  const int b = blockIdx.z;
  const unsigned* large = larges + (long)b * (F + 2);
  const unsigned nl = large[0] + 1u;
  if (nl == 0u) return;
  const float* nd = ndc + (long)b * V * 3;
  const int tx0 = blockIdx.x * RS_TILE, ty0 = blockIdx.y * RS_TILE;
  const int xi = tx0 + (threadIdx.x & 15), yi = ty0 + (threadIdx.x >> 4);
  unsigned long long best = RS_EMPTY;
  for (unsigned q = 0; q < nl; ++q) {
    const int fn = (int)large[1 + q];
    float f[9];
    load_face(nd, idx, fn, f);
    FaceEq e;
    if (!face_setup(f, is, e)) continue;
    int xa, xb, ya, yb;
    if (!face_box(e, is, xa, xb, ya, yb)) continue;
    if (xb < tx0 || xa > tx0 + RS_TILE - 1 || yb < ty0 || ya > ty0 + RS_TILE - 1) continue;     // (uniform over the workgroup)
    if (xi >= is || yi >= is) continue;
    const float zp = face_depth(e, xi, yi, is, near, far);
    if (zp < 0.f) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(zp) << 32) | (unsigned)fn;
    best = key < best ? key : best;
  }
  if (xi < is && yi < is && best != RS_EMPTY) {
    unsigned long long* z = &zbufs[(long)b * is * is + (long)yi * is + xi];
    if (best < *z) *z = best;
  }
}
// image = light of the winning face (0: background), rows flipped (rasterize.py: y up -> row 0 = top); the scratch is left empty
__global__ __launch_bounds__(256) void raster_resolve_kernel(unsigned long long* __restrict__ zbuf, const float* __restrict__ light, int is,
                                                             float* __restrict__ image, unsigned* __restrict__ large) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0) large[0] = 0xFFFFFFFFu;
  if (p >= is * is) return;
  const unsigned long long key = zbuf[p];
  const int yi = p / is, xi = p % is;
  image[(long)(is - 1 - yi) * is + xi] = key == RS_EMPTY ? 0.f : light[(unsigned)(key & 0xFFFFFFFFull)];
  zbuf[p] = RS_EMPTY;
}

// the same for render b = blockIdx.y of the mesh forms + what models/utils.py:108-125 does next, for the 2 x super-sampled render
// (anti_aliasing): 2 x 2 average (avg_pool2d: the window summed row by row, then / 4), optionally the x flip of models/utils.py:124
// (`[:, ::-1]`) and the white texture's three equal channels -> out [N,S,S] (channels == 1) or [N,S,S,3], S = is / 2.  fidx != NULL: also the
// face index of every super-sampled pixel [N,is,is] (z-buffer orientation, y up; -1 = background), which the backward reads.
__global__ __launch_bounds__(256) void raster_resolve_pool_kernel(unsigned long long* __restrict__ zbufs, const float* __restrict__ light, int F, int is,
                                                                  float* __restrict__ out, int* __restrict__ fidx, int flip_x, int channels,
                                                                  unsigned* __restrict__ larges) {
  const int S = is >> 1, b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0) larges[(long)b * (F + 2)] = 0xFFFFFFFFu;
  if (p >= S * S) return;
  unsigned long long* zbuf = zbufs + (long)b * is * is;
  const float* lt = light + (long)b * F;
  int* fi = fidx ? fidx + (long)b * is * is : nullptr;
  const int y = p / S, x = p % S;
  // the window's four keys first (independent loads in flight together), then their lights, summed in the order (dy, dx) = (0,0), (0,1), (1,0), (1,1)
  long q[4];
  unsigned long long key[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    q[k] = (long)(is - 1 - (2 * y + (k >> 1))) * is + 2 * x + (k & 1);       // image row r (0 = top) is z-buffer row is - 1 - r
    key[k] = zbuf[q[k]];
  }
  float l[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool bg = key[k] == RS_EMPTY;
    const unsigned face = (unsigned)(key[k] & 0xFFFFFFFFull);
    l[k] = bg ? 0.f : lt[face];
    if (fi) fi[q[k]] = bg ? -1 : (int)face;
    zbuf[q[k]] = RS_EMPTY;
  }
  const float acc = ((l[0] + l[1]) + l[2]) + l[3];
  const float v = acc / 4.f;
  const int xo = flip_x ? S - 1 - x : x;
  for (int ch = 0; ch < channels; ++ch) out[(((long)b * S + y) * S + xo) * channels + ch] = v;
}

// The launches of all three entry points: N renders of one topology at is x is, render b with its own ndc [V,3], z-buffer and large-face list
// (scratch = [N z-buffers][N x (F + 2) list words]).  v_world != NULL (the mesh forms, is = 2 S): ndc is projected from it (cam [N,12]) and the
// resolve pools.  v_world == NULL (the face-list form, N = 1): ndc holds the faces [F,9] themselves, idx is NULL and the resolve does not pool.
// (the coverage half is raster_coverage, which the textured entry point of avc_raster_tex.hip launches too)
void raster_coverage(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, int is, float near, float far,
                     const float* ndc, void* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* zbufs = (unsigned long long*)scratch;
  unsigned* larges = (unsigned*)(zbufs + (long)N * is * is);
  if (v_world) hipLaunchKernelGGL(raster_project_kernel, dim3((V + 255) / 256, N), dim3(256), 0, s, v_world, V, cam, width, const_cast<float*>(ndc));
  if (F) {
    hipLaunchKernelGGL(raster_faces_kernel, dim3((F + 3) / 4, N), dim3(256), 0, s, ndc, V, idx, F, is, near, far, zbufs, larges);
    const int nt = (is + RS_TILE - 1) / RS_TILE;
    hipLaunchKernelGGL(raster_large_kernel, dim3(nt, nt, N), dim3(256), 0, s, ndc, V, idx, F, is, near, far, zbufs, larges);
  }
}
static void raster_forward(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, const float* light, int is,
                           float near, float far, const float* ndc, float* out, int* fidx, int flip_x, int channels, void* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* zbufs = (unsigned long long*)scratch;
  unsigned* larges = (unsigned*)(zbufs + (long)N * is * is);
  raster_coverage(v_world, N, V, idx, F, cam, width, is, near, far, ndc, scratch, stream);
  if (v_world)
    hipLaunchKernelGGL(raster_resolve_pool_kernel, dim3((is / 2 * (is / 2) + 255) / 256, N), dim3(256), 0, s, zbufs, light, F, is, out, fidx, flip_x,
                       channels, larges);
  else
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((is * is + 255) / 256), dim3(256), 0, s, zbufs, light, is, out, larges);
}

extern "C" long avc_rasterize_scratch_bytes(int F, int image_size) {
  return (long)image_size * image_size * 8 + ((long)F + 2) * 4;
}
extern "C" int avc_rasterize_faces(const float* faces, const float* light, int F, int image_size, float near, float far,
                                   float* image, void* scratch, void* stream) {
  if (image_size <= 0) { avc_set_error("avc_rasterize_faces: image_size <= 0"); return 1; }
  if (F < 0 || near < 0.f) { avc_set_error("avc_rasterize_faces: F < 0 or near < 0"); return 1; }
  if (!image || !scratch || (F && (!faces || !light))) { avc_set_error("avc_rasterize_faces: NULL buffer"); return 1; }
  raster_forward(nullptr, 1, 0, nullptr, F, nullptr, 0.f, light, image_size, near, far, faces, image, nullptr, 0, 1, scratch, stream);
  return avc_check_launch("avc_rasterize_faces");
}
// The whole prior render of models/utils.py:108-125 from the world-space mesh: projection of the V vertices (cam = device [12]: eye + the
// look frame's x, y, z axes; width = tan(viewing angle)), the rasteriser above on faces gathered through idx [F,3] (fill_back copies
// included) at the 2 x super-sampled size 2 S, and the 2 x 2 average (+ x flip, + 3 equal channels) -> out [S,S(,3)].  ndc: [V,3] scratch.
extern "C" int avc_rasterize_mesh(const float* v_world, int V, const int* idx, int F, const float* cam, float width, const float* light,
                                  int S, float near, float far, float* ndc, float* out, int flip_x, int channels, void* scratch, void* stream) {
  if (S <= 0 || V <= 0 || F < 0 || near < 0.f || (channels != 1 && channels != 3)) { avc_set_error("avc_rasterize_mesh: bad sizes"); return 1; }
  if (!v_world || !cam || !ndc || !out || !scratch || (F && (!idx || !light))) { avc_set_error("avc_rasterize_mesh: NULL buffer"); return 1; }
  raster_forward(v_world, 1, V, idx, F, cam, width, light, 2 * S, near, far, ndc, out, nullptr, flip_x, channels, scratch, stream);
  return avc_check_launch("avc_rasterize_mesh");
}
// AvatarAnimate's batched form (mesh_render.py): N such renders in one call, render i with its own vertices, camera and light, one shared
// topology; no x flip, one channel, and the face-index map saved for avc_rasterize_mesh_grad (avc_raster_grad.hip)
extern "C" int avc_rasterize_mesh_save(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, const float* light,
                                       int S, float near, float far, float* ndc, float* image, int* fidx, void* scratch, void* stream) {
  if (N <= 0 || S <= 0 || V <= 0 || F < 0 || near < 0.f) { avc_set_error("avc_rasterize_mesh_save: bad sizes"); return 1; }
  if (!v_world || !cam || !ndc || !image || !fidx || !scratch || (F && (!idx || !light))) { avc_set_error("avc_rasterize_mesh_save: NULL buffer"); return 1; }
  raster_forward(v_world, N, V, idx, F, cam, width, light, 2 * S, near, far, ndc, image, fidx, 0, 1, scratch, stream);
  return avc_check_launch("avc_rasterize_mesh_save");
}
