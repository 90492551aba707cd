// Building blocks of the SDF + colour MLP kernels: one wavefront owns 32 points, every layer is a staged sequence of
// 32-row weight tiles (avc_stage.h).  See avc_common.h for the fragment layout.
// Follows AvatarGen/AppearanceGen/models/fields.py:72-107 (SDFNetwork.forward/.gradient) and :154-185
// (RenderingNetwork.forward, mode 'no_view_dir', extra_color) of the reference.
#pragma once
#include "avc_common.h"
#include "avc_stage.h"

template <int H_, int NMID_, int NCMID_>
struct NetT {
  static constexpr int H = H_;          // hidden width: 256 (confs/examples), 128 (confs/examples_small) or 64
  static constexpr int NMID = NMID_;    // HxH middle SDF layers: 2 | 1
  static constexpr int NCMID = NCMID_;  // HxH middle colour layers: 1 | 0
  static constexpr int HT = H / 32;     // 32-row output tiles of an H-wide layer
  static constexpr int HK = H / 16;     // 16-deep k-steps of an H-wide input
  static constexpr int SKIP = H - 39;   // width of the layer feeding the skip concat (fields.py:36-39)
  static constexpr int ST = (SKIP + 31) / 32;
  static constexpr int SK = 2 * ST;
  // whole 32-row tiles, and a skip layer left after the 39 PE inputs: the narrowest shape, H = 64, has HT = 2, ST = 1, SK = 2
  static_assert(H % 32 == 0 && SKIP > 0 && ST <= HT, "hidden width: a multiple of 32 above 39");
};
typedef NetT<256, 2, 1> NetFull;
typedef NetT<128, 1, 0> NetSmall;
typedef NetT<128, 2, 1> NetH128Deep;
typedef NetT<256, 1, 0> NetH256Shallow;
typedef NetT<64, 2, 1> NetH64Deep;
typedef NetT<64, 1, 0> NetH64Shallow;
// THE list of instantiated shapes: net id (include/avc.h: AVC_NET_*) -> type.  with_net(id, f) calls f(NetTag<N>{}) for the id's
// shape and returns its result, or `unknown` for an id outside the list; for_each_net(f) calls f for every shape (the launchers
// raise every instantiation's LDS limit once per device).  avatarclip_amd/packing.py: NET_IDS is the host's copy of this list
// and scripts/gen_offsets.py writes one Off<> per entry.
template <class N> struct NetTag { typedef N type; };
template <typename R, typename F>
static inline R with_net(int net, R unknown, F&& f) {
  switch (net) {
    case 0: return f(NetTag<NetFull>{});          // AVC_NET_FULL
    case 1: return f(NetTag<NetSmall>{});         // AVC_NET_SMALL
    case 2: return f(NetTag<NetH128Deep>{});      // AVC_NET_H128_DEEP
    case 3: return f(NetTag<NetH256Shallow>{});   // AVC_NET_H256_SHALLOW
    case 4: return f(NetTag<NetH64Deep>{});       // AVC_NET_H64_DEEP
    case 5: return f(NetTag<NetH64Shallow>{});    // AVC_NET_H64_SHALLOW
    default: return unknown;
  }
}
template <typename F>
static inline void for_each_net(F&& f) {
  for (int id = 0; with_net(id, false, [&](auto tag) { f(tag); return true; }); ++id) {}
}
#include "avc_offsets_gen.h"
// the launchers verify the table that came through the C ABI against the compiled-in one
template <class N> static inline bool offsets_match(const int* offs) {
  for (int k = 0; k < OFF_COUNT; ++k)
    if (offs[k] != Off<N>::value.v[k]) return false;
  return true;
}

struct PointSrc {
  const float* pts;      // [N,3] or nullptr -> ray mode
  const float* rays_o;   // [R,3]
  const float* rays_d;   // [R,3]
  const float* z;        // [R,ldz]
  int S;                 // samples per ray in this launch
  int ldz;
  int midpoint;          // 1: evaluate at section mid-points z + dist/2 (renderer.py:210-215)
  float sample_dist;
};

__device__ __forceinline__ void fetch_point(const PointSrc& ps, long i, float (&x)[3]) {
  if (ps.pts) {
    x[0] = ps.pts[3 * i]; x[1] = ps.pts[3 * i + 1]; x[2] = ps.pts[3 * i + 2];
    return;
  }
  const long ray = i / ps.S;
  const int s = (int)(i - ray * ps.S);
  const float* zr = ps.z + ray * ps.ldz;
  float t = zr[s];
  if (ps.midpoint) {
    const float dist = (s + 1 < ps.S) ? (zr[s + 1] - t) : ps.sample_dist;
    t = t + dist * 0.5f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = ps.rays_o[3 * ray + c] + ps.rays_d[3 * ray + c] * t;
}

template <typename V, int KS>
__device__ __forceinline__ const V* tptr(const V* blob, int off, int t, int lane) {
  return blob + (off >> 3) + (long)(t * KS) * 64 + lane;
}


// ---- tile geometry of every packed weight (k-steps per tile, tiles) ----
template <class N, int OFF> struct TileInfo;
#define AVC_TI(OFF, KS_, NT_) template <class N> struct TileInfo<N, OFF> { static constexpr int KS = KS_, NT = NT_; };
AVC_TI(OFF_W0, 3, N::HT)          AVC_TI(OFF_WM0, N::HK, N::HT)   AVC_TI(OFF_WM1, N::HK, N::HT)  AVC_TI(OFF_WS, N::HK, N::ST)
AVC_TI(OFF_WL, N::SK + 3, N::HT)  AVC_TI(OFF_W0T, N::HK, 2)       AVC_TI(OFF_WM0T, N::HK, N::HT) AVC_TI(OFF_WM1T, N::HK, N::HT)
AVC_TI(OFF_WST, N::SK, N::HT)     AVC_TI(OFF_WLT, N::HK, N::ST)   AVC_TI(OFF_C0, N::HK + 1, N::HT) AVC_TI(OFF_CM0, N::HK, N::HT)
AVC_TI(OFF_CH, N::HK, 1)          AVC_TI(OFF_C0T, N::HK, N::HT + 1) AVC_TI(OFF_CM0T, N::HK, N::HT) AVC_TI(OFF_CHT, 1, N::HT)
AVC_TI(OFF_W0G, 3, N::HT)

// descriptor of the FIRST group of packed weight OFF (what the layer before it prefetches)
template <class N, int OFF, class ST>
__device__ __forceinline__ Next nxt(const ST&, const void* blob, const AvcOffsets& o) {
  typedef TileInfo<N, OFF> TI;
  Next n;
  n.ptr = reinterpret_cast<const char*>(blob) + (long)o.v[OFF] * 2;
  constexpr int G = ST::template group<TI::KS>();
  // a group is 1 .. G whole tiles and fits one staging buffer, whatever the shape: thin layers (KS = 1 .. 5 at H = 64) do not get more
  // than ST::G tiles per group, layers with fewer tiles than a group (HT = 2, ST = 1) stage exactly their tiles
  static_assert(G >= 1 && G <= ST::G && TI::KS * 1024 * G <= ST::BUF_BYTES && TI::NT >= 1, "staging group of this layer");
  n.chunks = TI::KS * (TI::NT < G ? TI::NT : G);
  return n;
}
__device__ __forceinline__ Next no_next() { Next n; n.ptr = nullptr; n.chunks = 0; return n; }

// ---- staged, software-pipelined layer: per group one barrier + the DMA of the next group; inside a group tile t's MFMAs
// ---- are issued before the epilogue of tile t-1, so the VALU / transcendental / store work of one tile hides under the
// ---- matrix pipe of the next (same basic block, no barrier between).
// The two wavefronts of a SIMD (waves w and w+4 of the workgroup) leave every group barrier together and would run their MFMA
// chains at the same time and their VALU epilogues at the same time (matrix pipe idle during the epilogues).  (Holding the
// second wave back by about half a tile step with s_sleep, and a static s_setprio per wavefront, were measured and did not pay:
// profiles/r03_ab_kernels.txt.)
#define AVC_SYNC() __syncthreads()
#define AVC_EPI(...) [&](int t, const facc& acc) __attribute__((always_inline)) { __VA_ARGS__ }
// Optional hook run once per layer right AFTER the barrier of its first weight group: the place for streaming stores of the
// previous layer's output tiles (still live as this layer's input).  hipcc drains vmcnt(0) before every group barrier while an
// LDS-DMA is pending, and stores count on vmcnt: a store issued in an epilogue right before a barrier stalls the whole
// workgroup for an HBM write round trip; issued right after one it has a group of MFMA work (~2 us) to complete under.
struct NoHook { __device__ __forceinline__ void operator()() const {} };
#define AVC_HOOK(...) [&]() __attribute__((always_inline)) { __VA_ARGS__ }
// a hook that spreads its stores over the layer's tile steps: called with (t, number of tiles) and stores the t-th share of its
// tiles (tiles_store_part)
#define AVC_HOOKG(...) [&](int grp_, int ngrp_) __attribute__((always_inline)) { __VA_ARGS__ }
// A spreading hook is called once per output-TILE step with (t, NT), not once per weight group: its tile stores go out one tile (2 KiB
// per wavefront, 16 KiB per workgroup) at a time, each under ~500 cycles of MFMA work, instead of in bursts of 4 tiles behind a barrier
// (64 KiB per workgroup against a store path of 64 B/clk: the waves then sit on VMEM back-pressure).  profiles/r05_ab_kernels.txt:
// training forward 7.51 -> 7.45 ms, plain forward 5.88 -> 5.82 ms per 4 Mi points.  One-shot hooks (AVC_HOOK) run once, after the
// first barrier.
template <typename Hook>
__device__ __forceinline__ void hook_call(Hook&& hook, int g) {
  if constexpr (!std::is_invocable_v<Hook, int, int>) { if (g == 0) hook(); }
}
template <typename Hook>
__device__ __forceinline__ void hook_tile(Hook&& hook, int t, int nt) {
  if constexpr (std::is_invocable_v<Hook, int, int>) hook(t, nt);
}

// ---- THE walk: the one place where the schedule above is written down.  Every layer form below is a wrapper of it.
//   mma(j, t, two, a0, a1)  runs the chain of output tile t (tile j of the staged group) into a0 and, when `two`, that of tile t + 1 into a1
//   pre(t)                  AVC_PRE: the global loads the epilogue of tile t needs, returned raw; NoPre: there are none
//   epi(t, acc, data)       the epilogue of tile t (AVC_EPID); with NoPre it is epi(t, acc) (AVC_EPI)
// PAIRED = two output tiles per MFMA stream.  Measured per 4 Mi points (profiles/r03_ab_kernels.txt): forward 6.16 -> 6.01 ms and
// training forward 8.25 -> 7.84 ms with it (and 26 / 36 spilled registers become 0 / 12); the SDF-only kernel loses 6 % (its 168
// registers leave no room for the second accumulator: 16 -> 28 spills) and the backward kernel 3 %: those keep one chain
// (layer_s1, layer_sq1); the forward kernels pair everywhere (layer_s, layer_sq, layer2_s).
// Loads one chain ahead: the loads of the pending epilogue(s) (panel tiles read back by the sweeps) go out BEFORE the chain(s) of the
// current step and are consumed after them.  The backward kernel keeps only ~16 KiB of reads in flight per CU when every epilogue
// loads and immediately waits; one chain (~600 cycles) of head start costs no extra live set beyond the loaded registers themselves.
// (pre(t) before the chain of tile t itself -- two chains + one epilogue of head start, two load sets live -- measured slower for the
// three-array loads of the reverse sweep: register pressure)
#define AVC_PRE(...) [&](int t) __attribute__((always_inline)) { __VA_ARGS__ }
#define AVC_EPID(DT, ...) [&](int t, const facc& acc, const DT& d) __attribute__((always_inline)) { __VA_ARGS__ }
struct NoPre { __host__ __device__ __forceinline__ int operator()(int) const { return 0; } };   // (__host__: its result type is asked for outside device code)
template <bool PAIRED, int KS, int NT, class ST, typename V, typename Mma, typename Pre, typename Epi, typename Hook>
__device__ __forceinline__ void layer_walk(ST& st, const V* __restrict__ blob, int offw, const Next& after, Mma&& mma, Pre&& pre,
                                           Epi&& epi, Hook&& hook) {
  constexpr int G = ST::template group<KS>();
  constexpr int NG = (NT + G - 1) / G;
  constexpr bool LOADS = !std::is_same_v<std::decay_t<Pre>, NoPre>;
  typedef std::invoke_result_t<Pre&, int> D;
  auto finish = [&](int t, const facc& acc, const D& d) __attribute__((always_inline)) {
    if constexpr (LOADS) epi(t, acc, d);
    else epi(t, acc);
  };
  facc prev0, prev1;
  D d0{}, d1{};
  int tp = -1, np = 0;   // first tile / number of tiles whose epilogue is pending (compile-time after unrolling)
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    AVC_SYNC();   // group g has landed (hipcc drains vmcnt before the barrier); the other buffer is free
    if (g + 1 < NG) {
      Next n;
      n.ptr = blob + (offw >> 3) + (long)((g + 1) * G * KS) * 64;
      n.chunks = KS * ((NT - (g + 1) * G) < G ? (NT - (g + 1) * G) : G);
      stage_issue(st, n, st.par ^ 1);
    } else {
      stage_issue(st, after, st.par ^ 1);
    }
    hook_call(hook, g);
#pragma unroll
    for (int j = 0; j < G; j += (PAIRED ? 2 : 1)) {
      const int t = g * G + j;
      if (t < NT) {
        const bool two = PAIRED && (j + 1 < G) && (t + 1 < NT);
        hook_tile(hook, t, NT);
        if (two) hook_tile(hook, t + 1, NT);
        if (LOADS && np > 0) {
          d0 = pre(tp);
          if (np > 1) d1 = pre(tp + 1);
          __builtin_amdgcn_sched_barrier(0);   // the loads go out before the chains
        }
        facc a0, a1;
        mma(j, t, two, a0, a1);
        if (np > 0) {
          finish(tp, prev0, d0);
          if (np > 1) finish(tp + 1, prev1, d1);
          if (two) { interleave_mfma_valu<KS>(); interleave_mfma_valu<KS>(); } else interleave_mfma_valu<KS>();
        }
        prev0 = a0;
        if (two) prev1 = a1;
        tp = t; np = two ? 2 : 1;
        __builtin_amdgcn_sched_barrier(0);   // keep epilogues from being sunk past later tiles
      }
    }
    st.par ^= 1;
  }
  if constexpr (LOADS) {
    d0 = pre(tp);
    if (np > 1) d1 = pre(tp + 1);
  }
  finish(tp, prev0, d0);
  if (np > 1) finish(tp + 1, prev1, d1);
  __builtin_amdgcn_sched_barrier(0);
}
// one input array: the shared wrapper of the four forms below
template <bool PAIRED, typename V, int KS, int NT, class ST, typename Pre, typename Epi, typename Hook, class Bias>
__device__ __forceinline__ void layer_sp(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&in)[KS],
                                         Pre&& pre, Epi&& epi, Hook&& hook, const Bias& bias) {
  layer_walk<PAIRED, KS, NT>(st, blob, offw, after, [&](int j, int t, bool two, facc& a0, facc& a1) __attribute__((always_inline)) {
    if (two) tile_mma_pair<V, KS>(st, j, in, a0, a1, bias, t);
    else a0 = tile_mma<V, KS>(st, j, in, bias, t);
  }, pre, epi, hook);
}
template <typename V, int KS, int NT, class ST, typename Epi, typename Hook = NoHook, class Bias = NoBias>
__device__ __forceinline__ void layer_s(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&in)[KS],
                                        Epi&& epi, Hook&& hook = NoHook{}, const Bias& bias = NoBias{}) {
  layer_sp<true, V, KS, NT>(st, blob, offw, after, in, NoPre{}, epi, hook, bias);
}
template <typename V, int KS, int NT, class ST, typename Epi, typename Hook = NoHook, class Bias = NoBias>
__device__ __forceinline__ void layer_s1(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&in)[KS],
                                         Epi&& epi, Hook&& hook = NoHook{}, const Bias& bias = NoBias{}) {
  layer_sp<false, V, KS, NT>(st, blob, offw, after, in, NoPre{}, epi, hook, bias);   // always one accumulator chain
}
template <typename V, int KS, int NT, class ST, typename Pre, typename Epi, typename Hook = NoHook>
__device__ __forceinline__ void layer_sq(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&in)[KS],
                                         Pre&& pre, Epi&& epi, Hook&& hook = NoHook{}) {
  layer_sp<true, V, KS, NT>(st, blob, offw, after, in, pre, epi, hook, NoBias{});
}
template <typename V, int KS, int NT, class ST, typename Pre, typename Epi, typename Hook = NoHook>
__device__ __forceinline__ void layer_sq1(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&in)[KS],
                                          Pre&& pre, Epi&& epi, Hook&& hook = NoHook{}) {
  layer_sp<false, V, KS, NT>(st, blob, offw, after, in, pre, epi, hook, NoBias{});   // always one accumulator chain
}
// the K dimension split over two input arrays (tiles of KA + KB k-steps)
template <typename V, int KA, int KB, int NT, class ST, typename Epi, typename Hook = NoHook, class Bias = NoBias>
__device__ __forceinline__ void layer2_s(ST& st, const V* __restrict__ blob, int offw, const Next& after, const V (&ina)[KA],
                                         const V (&inb)[KB], Epi&& epi, Hook&& hook = NoHook{}, const Bias& bias = NoBias{}) {
  layer_walk<true, KA + KB, NT>(st, blob, offw, after, [&](int j, int t, bool two, facc& a0, facc& a1) __attribute__((always_inline)) {
    if (two) tile_mma2_pair<V, KA, KB>(st, j, ina, inb, a0, a1, bias, t);
    else a0 = tile_mma2<V, KA, KB>(st, j, ina, inb, bias, t);
  }, NoPre{}, epi, hook);
}

// ---------------------------------------------------------------------------------------------------------------
// Operand panels of the training path (mirrored by packing.py: build_layout).  Every operand of every weight-gradient
// product is stored ONCE, in the layout the producing wavefront holds it in: per 32-point block and 32-feature tile the two
// B-operand fragments [k-step e][lane][8 x 16 bit] (lane = point + 32 * half), 2 KiB per tile.  Two REGIONS with their own
// block stride:
//   F region (P_* indices, P_TILES tiles per block): forward-type operands (h, g_a, feature, r, [x,n], PE), f16, written by
//            the forward kernel for every block of the ray set and kept until the backward pass;
//   G region (G_* indices, G_TILES tiles per block): gradient-type operands (gbar_h, abar, delta, ybar), bf16, written by the
//            backward kernel.  The backward pass walks the ray set in SLABS (backward kernel + weight-gradient kernel per
//            slab), so the G region holds one slab and is reused: the gradient-type half of the operands never exists for
//            more than a slab at a time (512^2 x 64 spp: 87 GiB of F panels + 23 GiB of G panels instead of 177 GiB).
// The sweeps of both kernels read tiles back as they are (no transposition), the weight-gradient kernel transposes them with
// the LDS transpose read when it loads them (avc_wgrad.hip).
// ---------------------------------------------------------------------------------------------------------------
template <class N>
struct PanelLayout {
  static constexpr int HT = N::HT, ST = N::ST, NM = N::NMID, NC = N::NCMID;
  // ---- F region.  (hs, pe) are adjacent: the last layer's input is [hs | pe], so its weight-gradient product reads them as
  // ONE run of ST + 2 tiles; (feature, [x,n]) likewise for the first colour layer
  static constexpr int P_H1 = 0;                    // h1
  static constexpr int P_HM = P_H1 + HT;            // hm[NM]
  static constexpr int P_HS = P_HM + NM * HT;       // hs (ST)
  static constexpr int P_H0 = P_HS + ST;            // pe values (2 tiles)
  static constexpr int P_GA1 = P_H0 + 2;            // g_a1
  static constexpr int P_GAM = P_GA1 + HT;          // g_am[NM]
  static constexpr int P_GAS = P_GAM + NM * HT;     // g_as (ST)
  static constexpr int P_FEAT = P_GAS + ST;         // feature (HT)
  static constexpr int P_XN = P_FEAT + HT;          // [x, n] (1)
  static constexpr int P_R1 = P_XN + 1;             // r1 (HT)
  static constexpr int P_R2 = P_R1 + HT;            // r2 (HT, only NC==1)
  static constexpr int P_TILES = P_R2 + NC * HT;    // tiles per block of the F region
  // ---- G region.  (ybar[1:], d_sdf) are adjacent for the same reason.  gbar_hs has NO panel: its only consumers are the first layer of
  // the reverse sweep (which takes it from the registers of the second-order sweep) and the column sum over the points that is the
  // second-order term of row 0 of the last layer (reduced in the backward kernel: col_sums in csrc/avc_bwd_body.h) -- rounds 2-4 wrote it,
  // and a constant-one tile, for a "1 (x) [gbar_hs | gbar_h0]" product in the weight-gradient kernel: 8 tiles written + 10 read per block
  static constexpr int G_GBH1 = 0;                  // gbar_h1
  static constexpr int G_GBHM = G_GBH1 + HT;        // gbar_hm[NM]
  static constexpr int G_GB0 = G_GBHM + NM * HT;    // gbar_h0 (2)
  static constexpr int G_AB1 = G_GB0 + 2;           // abar_1
  static constexpr int G_ABM = G_AB1 + HT;          // abar_m[NM]
  static constexpr int G_ABS = G_ABM + NM * HT;     // abar_s (ST)
  static constexpr int G_DFEAT = G_ABS + ST;        // ybar[1:] (HT)
  static constexpr int G_SDF = G_DFEAT + HT;        // feature 0 = d_sdf (1)
  static constexpr int G_D1 = G_SDF + 1;            // delta1 (HT)
  static constexpr int G_D2 = G_D1 + HT;            // delta2 (HT, only NC==1)
  static constexpr int G_DO = G_D2 + NC * HT;       // delta_o (1)
  static constexpr int G_TILES = G_DO + 1;          // tiles per block of the G region
  static constexpr int MASK_U16 = 2 * HT * 64;      // ReLU masks of r1 / r2 per 32-point block: [layer][tile][lane] x 16 bits
  static constexpr int CS_FLOATS = ST * 32 + 48;    // column sums per wavefront: [ST][2 halves][16 acc registers] of gbar_hs, [3 frags][2][8 slots] of gbar_h0
};
// the no-grad forward parks only what its own normal sweep reads back (h1, hm, feature), in a per-wavefront slot it reuses
template <class N>
struct ScratchLayout {
  static constexpr int HT = N::HT, NM = N::NMID;
  static constexpr int P_H1 = 0, P_HM = HT, P_FEAT = HT + NM * HT, P_TILES = P_FEAT + HT;
  static constexpr int P_H0 = 0, P_HS = 0, P_GA1 = 0, P_GAM = 0, P_GAS = 0, P_XN = 0, P_R1 = 0, P_R2 = 0;   // never written
};

// Panel addressing: `ub` = wave-uniform base of the block's panels (SGPR pair), `off` = lane * 16 (ONE VGPR shared by every
// access); the tile base is formed on the scalar unit and kept opaque, so that hipcc emits the saddr form
// (global_store v_off, v_data, s[base]) instead of one 64-bit VGPR address pair per tile (those pairs were being
// computed early and spilled: +130 spilled registers in the training forward kernel).
struct PanelPtr {
  AVC_GLOBAL char* ub;
  unsigned off;
};
__device__ __forceinline__ PanelPtr panel_ptr(char* base, int lane) {
  const unsigned long long v = (unsigned long long)base;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  PanelPtr p;
  p.ub = (AVC_GLOBAL char*)(((unsigned long long)hi << 32) | lo);
  p.off = (unsigned)lane * 16u;
  return p;
}
template <typename V> __device__ __forceinline__ AVC_GLOBAL V* tile_addr(const PanelPtr& pp, int tile) {
  AVC_GLOBAL char* tb = pp.ub + (long)tile * 2048;
  asm("" : "+s"(tb));
  return (AVC_GLOBAL V*)(tb + pp.off);
}
// an all-zero fragment: the second half of an operand tile that has one k-step of content
template <typename V>
__device__ __forceinline__ V zero_frag() {
  V z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (typename MF<V>::S)0.f;
  return z;
}
// KEEP = read back soon by the same kernel (normal cache policy), otherwise streamed past the caches (consumed by a later launch)
// (No predicate: wavefronts past the end of the point set write to the SINK block that follows the last real block of the
// panel buffer -- a branch around every store splits the scheduling regions of the epilogues and costs ~110 spilled registers.)
template <bool KEEP, typename V>
__device__ __forceinline__ void tile_store(const PanelPtr& pp, int tile, const V& f0, const V& f1) {
  AVC_GLOBAL V* p = tile_addr<V>(pp, tile);
  if (KEEP) {
    p[0] = f0;
    p[64] = f1;
  } else {
    AVC_NT_STORE(f0, &p[0]);
    AVC_NT_STORE(f1, &p[64]);
  }
}
// all tiles of one activation (fragment array `f`, 2 per tile) in one go -- what the hooks above issue
template <bool KEEP, int NT, typename V, int KS>
__device__ __forceinline__ void tiles_store(const PanelPtr& pp, int tile0, const V (&f)[KS]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) tile_store<KEEP>(pp, tile0 + t, f[2 * t], f[2 * t + 1]);
}
// the g-th of ng shares of the tiles of one activation (g, ng compile-time after unrolling: the tile test folds)
template <bool KEEP, int NT, typename V, int KS>
__device__ __forceinline__ void tiles_store_part(const PanelPtr& pp, int tile0, const V (&f)[KS], int g, int ng) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t * ng / NT == g) tile_store<KEEP>(pp, tile0 + t, f[2 * t], f[2 * t + 1]);
}
template <typename V> struct FragPair { V a0, a1; };     // the two k-step fragments of a panel tile
template <bool NT, typename V>
__device__ __forceinline__ FragPair<V> tile_load(const PanelPtr& pp, int tile) {
  const AVC_GLOBAL V* p = tile_addr<V>(pp, tile);
  FragPair<V> d;
  if (NT) { d.a0 = AVC_NT_LOAD(&p[0]); d.a1 = AVC_NT_LOAD(&p[64]); }
  else { d.a0 = p[0]; d.a1 = p[64]; }
  return d;
}

// SDF value only (avc_sdf_forward): same layers as sdf_trunk but every activation array dies as soon as the next layer
// has consumed it, which keeps the kernel at two wavefronts per SIMD.
#define AVC_SDF_ACT(OUT)                                                                      \
  AVC_EPI(float a[16];                                                                        \
          softplus2_tile(acc, a);                                                             \
          acc_to_frags(a, OUT[2 * t], OUT[2 * t + 1]);)
template <class N, class ST, typename TP>
__device__ __forceinline__ float sdf_only(ST& sg, const h8* __restrict__ Wf, TP T, const AvcOffsets& o,
                                          int h, const float (&x)[3]) {
  PE pe;
  pe_compute(x, h, pe);
  float part = 0.f;
  {
    const auto wpe = T + o.v[OFF_WL0_PE] + h * 24;
#pragma unroll
    for (int q = 0; q < 24; ++q) part += wpe[q] * pe.v[q];
    asm volatile("" : "+v"(part));   // done HERE (hipcc otherwise sinks the fmacs to the first use of `part` and keeps their operands alive)
  }
  h8 hlast[N::HK];
  {
    h8 h1[N::HK];
    {
      h8 pef[3];
      pe_to_frags_f16(pe, x, h, pef);
      layer_s1<h8, 3, N::HT>(sg, Wf, o.v[OFF_W0], nxt<N, OFF_WM0>(sg, Wf, o), pef, AVC_SDF_ACT(h1),
                             NoHook{}, TabBias{T + o.v[OFF_B0], h});
    }
    h8 hm0[N::HK];   // between the two middle layers (NMID == 2)
    layer_s1<h8, N::HK, N::HT>(sg, Wf, o.v[OFF_WM0], nxt<N, (N::NMID == 2 ? OFF_WM1 : OFF_WS)>(sg, Wf, o), h1,
                               AVC_SDF_ACT((N::NMID == 2 ? hm0 : hlast)), NoHook{}, TabBias{T + o.v[OFF_BM0], h});
    if constexpr (N::NMID == 2)
      layer_s1<h8, N::HK, N::HT>(sg, Wf, o.v[OFF_WM1], nxt<N, OFF_WS>(sg, Wf, o), hm0, AVC_SDF_ACT(hlast),
                                 NoHook{}, TabBias{T + o.v[OFF_BM1], h});
  }
  layer_s1<h8, N::HK, N::ST>(sg, Wf, o.v[OFF_WS], no_next(), hlast, AVC_EPI(
    float w[16];
    load16(T + o.v[OFF_WL0_ACC], t, h, w);
    _Pragma("unroll") for (int r = 0; r < 16; ++r) part += w[r] * softplus2(acc[r]);
  ), NoHook{}, TabBias{T + o.v[OFF_BS], h});
  return xhalf_sum(part) + T[o.v[OFF_BL0]];
}
#undef AVC_SDF_ACT
