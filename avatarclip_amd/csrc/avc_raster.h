// Device helpers shared by the forward rasteriser (avc_raster.hip) and its pseudo-gradient (avc_raster_grad.hip): the face set-up, edge / depth test, box and gather of the nine floats of a face, and the look + perspective
// projection of one vertex.  Both translation units compile them under `fp contract(off)`: the edge tests are sign tests and the
// backward's scan-line crossings are floored / ceiled, so every rounding must be the one the fp32 restatements make.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define RS_EMPTY 0xFFFFFFFFFFFFFFFFull
#define RS_LARGE 1024     // pixels in a face's box from which it goes to the tile-parallel pass
#define RS_TILE 16

// depth of face (x0..z2) at pixel (xi, yi), or a negative number if the pixel centre is outside / the depth out of range
struct FaceEq {
  float x0, y0, z0, x1, y1, z1, x2, y2, z2;
  float p0x, p0y, p1x, p1y, p2x, p2y, den;
};
__device__ __forceinline__ bool face_setup(const float* __restrict__ f, int is, FaceEq& e) {
  e.x0 = f[0]; e.y0 = f[1]; e.z0 = f[2]; e.x1 = f[3]; e.y1 = f[4]; e.z1 = f[5]; e.x2 = f[6]; e.y2 = f[7]; e.z2 = f[8];
  if ((e.y2 - e.y0) * (e.x1 - e.x0) < (e.y1 - e.y0) * (e.x2 - e.x0)) return false;          // back-facing
  // pixel-space vertices and the inverse of their homogeneous matrix (rasterize_cuda_kernel.cu, kernel 1)
  e.p0x = 0.5f * (e.x0 * is + is - 1); e.p0y = 0.5f * (e.y0 * is + is - 1);
  e.p1x = 0.5f * (e.x1 * is + is - 1); e.p1y = 0.5f * (e.y1 * is + is - 1);
  e.p2x = 0.5f * (e.x2 * is + is - 1); e.p2y = 0.5f * (e.y2 * is + is - 1);
  e.den = e.p2x * (e.p0y - e.p1y) + e.p0x * (e.p1y - e.p2y) + e.p1x * (e.p2y - e.p0y);
  return e.den != 0.f;
}
// the clamped barycentric weights w of pixel (xi, yi), their sum ws (at least 1e-10; w / ws = the normalised weights) and the perspective-correct
// depth zp: what face_depth tests and the textured resolve (avc_raster_tex.hip) samples with; false: the pixel centre is outside the face
__device__ __forceinline__ bool face_weights(const FaceEq& e, int xi, int yi, int is, float (&w)[3], float& ws, float& zp) {
  const float xp = (2.f * xi + 1.f - is) / is;
  const float yp = (2.f * yi + 1.f - is) / is;
  if (((yp - e.y0) * (e.x1 - e.x0) < (xp - e.x0) * (e.y1 - e.y0)) || ((yp - e.y1) * (e.x2 - e.x1) < (xp - e.x1) * (e.y2 - e.y1)) ||
      ((yp - e.y2) * (e.x0 - e.x2) < (xp - e.x2) * (e.y0 - e.y2)))
    return false;
  float w0 = ((e.p1y - e.p2y) * xi + (e.p2x - e.p1x) * yi + (e.p1x * e.p2y - e.p2x * e.p1y)) / e.den;
  float w1 = ((e.p2y - e.p0y) * xi + (e.p0x - e.p2x) * yi + (e.p2x * e.p0y - e.p0x * e.p2y)) / e.den;
  float w2 = ((e.p0y - e.p1y) * xi + (e.p1x - e.p0x) * yi + (e.p0x * e.p1y - e.p1x * e.p0y)) / e.den;
  w0 = fminf(fmaxf(w0, 0.f), 1.f); w1 = fminf(fmaxf(w1, 0.f), 1.f); w2 = fminf(fmaxf(w2, 0.f), 1.f);
  ws = fmaxf(w0 + w1 + w2, 1e-10f);
  zp = 1.f / ((w0 / e.z0 + w1 / e.z1 + w2 / e.z2) / ws);
  w[0] = w0; w[1] = w1; w[2] = w2;
  return true;
}
__device__ __forceinline__ float face_depth(const FaceEq& e, int xi, int yi, int is, float near, float far) {
  float w[3], ws, zp;
  if (!face_weights(e, xi, yi, is, w, ws, zp)) return -1.f;
  return (zp > near && zp < far) ? zp : -1.f;        // (zp > near >= 0: its bit pattern orders like its value)
}
// the face's box in pixel indices, one pixel of slack each way (the edge functions decide); false: off screen (or NaN)
__device__ __forceinline__ bool face_box(const FaceEq& e, int is, int& xa, int& xb, int& ya, int& yb) {
  const float xl = fminf(e.x0, fminf(e.x1, e.x2)), xh = fmaxf(e.x0, fmaxf(e.x1, e.x2));
  const float yl = fminf(e.y0, fminf(e.y1, e.y2)), yh = fmaxf(e.y0, fmaxf(e.y1, e.y2));
  if (!(xh >= -1.f && xl <= 1.f && yh >= -1.f && yl <= 1.f)) return false;
  // (clamped in float first: a vertex near the camera plane projects to 1e30, which no int holds)
  xa = max(0, (int)floorf(fmaxf(0.5f * (xl * is + is - 1), -1.f)) - 1); xb = min(is - 1, (int)ceilf(fminf(0.5f * (xh * is + is - 1), (float)is)) + 1);
  ya = max(0, (int)floorf(fmaxf(0.5f * (yl * is + is - 1), -1.f)) - 1); yb = min(is - 1, (int)ceilf(fminf(0.5f * (yh * is + is - 1), (float)is)) + 1);
  return xb >= xa && yb >= ya;
}

// the nine floats of face fn: from faces [F,9], or (idx != NULL) gathered from the projected vertices faces = ndc [V,3] through idx [F,3]
__device__ __forceinline__ void load_face(const float* __restrict__ faces, const int* __restrict__ idx, int fn, float (&f)[9]) {
  if (idx) {
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      const long vi = idx[3 * (long)fn + v];
#pragma unroll
      for (int k = 0; k < 3; ++k) f[3 * v + k] = faces[3 * vi + k];
    }
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = faces[(long)fn * 9 + k];
  }
}
// neural_renderer's look + perspective (look.py, perspective.py; models/utils.py:108-125): v_cam = (v - eye) . (x, y, z axes),
// ndc = (x / z / width, y / z / width, z), (0, 0, 0) for z <= 0; cam = [12]: eye, x axis, y axis, z axis
__device__ __forceinline__ void project_vertex(const float* __restrict__ vw, int i, const float* __restrict__ cam, float width,
                                               float* __restrict__ ndc) {
  const float d0 = vw[3 * i] - cam[0], d1 = vw[3 * i + 1] - cam[1], d2 = vw[3 * i + 2] - cam[2];
  float c[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) c[j] = fmaf(d2, cam[3 + 3 * j + 2], fmaf(d1, cam[3 + 3 * j + 1], d0 * cam[3 + 3 * j]));
  const bool behind = c[2] <= 0.f;      // the patch the reference's README.md:126-134 prescribes for perspective.py: behind the camera -> (0, 0, 0)
  ndc[3 * i] = behind ? 0.f : c[0] / c[2] / width;
  ndc[3 * i + 1] = behind ? 0.f : c[1] / c[2] / width;
  ndc[3 * i + 2] = behind ? 0.f : c[2];
}

// The coverage launches every forward entry point shares (avc_raster.hip): the projection (v_world != NULL: cam [N,12] -> ndc [N,V,3]), one
// wavefront per face and the tile pass of the large faces.  They leave the winners' (depth, face) keys in the N z-buffers of `scratch`
// ([N z-buffers][N x (F + 2) list words]); a resolve launch reads them and puts the all-ones "empty" key and list count back.
void raster_coverage(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, int is, float near, float far,
                     const float* ndc, void* scratch, void* stream);
