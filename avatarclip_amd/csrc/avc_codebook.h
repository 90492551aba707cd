/* avc_codebook.h -- the k-means entry points of libavc.so (csrc/avc_codebook.hip), a third part of the C ABI of include/avc.h.
 *
 * Same conventions as include/avc.h: every pointer is a DEVICE pointer, buffers are caller-allocated, `stream` is a hipStream_t, the calls
 * enqueue and return without synchronising, 0 = ok, otherwise avc_last_error() describes the failure.  The interface revision is that header's
 * AVC_ABI_VERSION (4; avc_version() reports it): added entry points do not change it.  avatarclip_amd/lib.py parses the three headers and
 * binds the union of their prototypes.
 *
 * The reference ships the two codebooks these build (AvatarGen/ShapeGen/main.py:86-91 and AvatarAnimate/models/pose_generation.py:298-300
 * only load them); the paper makes them by K-Means.  avatarclip_amd/kmeans.py is Lloyd's loop around the two calls.
 */
#ifndef AVC_CODEBOOK_H
#define AVC_CODEBOOK_H
#ifdef __cplusplus
extern "C" {
#endif

/* Nearest centre of every point.  x [N,D] and c [K,D] fp32, D = 16 or 32 (anything else: an error status), 1 <= N, N D < 2^31,
 * 1 <= K <= 65536.  dist[i] = min over k of sum over d ascending of (x[i,d] - c[k,d])^2, the direct form, one fp32 chain per (point, centre)
 * with a fused multiply-add per term; assign[i] = the LOWEST k that attains it (the centres are walked in ascending k and a later one must be
 * strictly nearer).  A point equal to a centre has dist exactly 0.  Inputs are finite (a NaN distance never wins: such a point keeps k = 0
 * and dist = +inf). */
int avc_kmeans_assign(const float* x, int N, int D, const float* c, int K, int* assign, float* dist, void* stream);
/* The mean of every cluster.  sorted [N]: the words (assign[i] << 32) | i in ascending order (the caller sorts them, any sort: they are
 * distinct), so cluster k is a run whose point indices ascend.  counts[k] = the number of points in k's run (int32, all K written).  A cluster with
 * points: c[k,d] = s / (float)counts[k], s the fp32 sum of x[i,d] over the run taken SEQUENTIALLY in ascending point index from 0.0f, the
 * division correctly rounded.  A cluster without points keeps c[k,:] bit for bit.  c is updated in place.  No atomics of any kind: the
 * same input gives the same bits.  Words naming k >= K or i >= N are skipped. */
int avc_kmeans_update(const long long* sorted, int N, const float* x, int D, float* c, int K, int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
