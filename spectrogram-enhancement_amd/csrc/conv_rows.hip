// conv_rows.hip — the encoder's pooled 5 x 5 convolutions as a row sweep (gfx950).
//
// VAE/manual_scan_3layers.py:188-193: Conv2D(32, 5, relu, same) + MaxPooling2D(2) on the
// 64 x 64 x 16 map, Conv2D(64, 5, relu, same) + MaxPooling2D(2) on the 32 x 32 x 32 map.
// conv_patch_kernel (conv_ae.hip) runs these as 16 x 16 output tiles: every patch fragment
// feeds the MFMAs of ONE (tap, output row) and every tile re-stages a 2-pixel halo; PMC put
// both layers at 0.31-0.41 of the MFMA peak with ~5 VALU + 2.5 SALU instructions per MFMA.
// Here a workgroup walks whole images DOWN, two input rows per step:
//  * wave (window wx, channel block nb) owns 16 output columns x 16 output channels. Its 25
//    (CIN = 32) or 13 (CIN = 16, two taps per K = 32 step) weight fragments stay in registers
//    for the whole launch (the MFMA A operand: 16 output channels x 32 K).
//  * input row r is read ONCE per (window, tap column): that B fragment (32 K x 16 pixels)
//    feeds the MFMAs of all five kernel rows, i.e. output rows r + 2 - ky (5 MFMAs per LDS
//    read). Six accumulators (output rows 2q - 2 .. 2q + 3) rotate down the image.
//  * CIN = 16 pairs taps (kx, kx + 1) of one input row in a K step (columns 0-1, 2-3); the
//    fifth column pairs rows: F(r) = (row r, row r + 1) at kx = 4 feeds output rows r + 2
//    (weights w[0][4], w[1][4]), r (w[2][4], w[3][4]) and r - 2 (w[4][4], 0): 13 MFMAs per
//    input row for 12.5 taps of work (plus F(-1) once per image for output row 1).
//  * when output rows 2p, 2p + 1 are complete, the 2 x 2 max-pool runs in registers (rows in
//    lane, columns across the lane pair m, m ^ 1 by DPP); the bias is the accumulators'
//    start value and ReLU / rounding commute with the max, so pooled row p is
//    round_T(relu(max)) and is stored as 8 bytes per even lane.
//  * input rows arrive by LDS-DMA (global_load_lds, 16 B per lane) into an 8-row ring,
//    three steps ahead; rows outside the image are zero-filled, as is the 2-pixel halo of
//    every ring row. One workgroup barrier per step. Workgroups are persistent: the row
//    stream runs on across the workgroup's images (image i, rows 0 .. H + 1, the last two
//    zero), so the pipeline never drains between images.
// 64-byte pixels (CIN = 32) are stored with their 16-byte groups swizzled, g ^ ((p >> 1) & 3)
// (conflict-free B-fragment reads under the ds_read_b128 lane groups); 32-byte pixels need
// no swizzle. Host-checked shapes: (CIN, COUT, W) = (16, 32, 64) and (32, 64, 32), H even.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>

#include "lds_dma.hpp"
#include "mma.hpp"
#include "specenh.h"
#include "runtime.hpp"
#include "wave.hpp"

namespace specenh {

namespace {

// max with the neighbouring lane (m ^ 1): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float max_pair(float v) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));
  return fmaxf(v, o);
}

template <int CIN, int COUT, int W, int K = 5>
struct RC {
  static constexpr int NWIN = W / 16;                 // 16-column windows
  static constexpr int NNB = COUT / 16;               // 16-channel blocks
  static constexpr int WAVES = NWIN * NNB;
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int PIX = CIN * 2;                 // bytes per pixel
  static constexpr int ROWB = (W + 4) * PIX;          // ring row: 2 zero pixels each side
  static constexpr int RING = 8;                      // rows (4 steps)
  // The step timeline's constants (restated and checked on the host by
  // tests/test_conv_rows_sched_model.py): a step issues the DMA of the rows LEAD steps ahead
  // and waits at its end for the DMA issued one step earlier (rows LEAD - 1 ahead); the
  // prefetching schedule (SCHED = 1) reads the fragments of the step PF ahead.
  static constexpr int LEAD = 3;
  static constexpr int PF = 1;
  static_assert(2 * (LEAD + 1) <= RING && PF < LEAD - 1, "ring slots live: steps s - 1 + PF .. s + LEAD");
  static constexpr int LDS = RING * ROWB;
  static constexpr int NW = CIN == 16 ? 13 : K * K;   // resident weight fragments
  static_assert(K == 5 || (CIN == 32 && (K == 3 || K == 5)), "kernel size");
  static constexpr int CPP = CIN / 8;                 // 16-byte groups per pixel
  static constexpr int CHUNKS = W * CPP;              // 16-byte chunks per row
  static constexpr int WPR = CHUNKS / 64;             // waves moving one row (1 KB each)
  static constexpr int DMA_WAVES = 2 * WPR;           // waves moving a step's two rows
  static_assert(WAVES == 8 && CHUNKS % 64 == 0 && DMA_WAVES <= WAVES, "shape");
  // waves per SIMD the register budget is sized for (CIN = 32 holds K^2 fragments)
  static constexpr int WPE = CIN == 16 || K == 3 ? 4 : 2;
};

struct CRArgs {
  const void* x;     // [N][H][W][CIN]
  const void* w;     // forward GEMM weights [COUT][5][5][CIN]
  const float* b;    // [COUT]
  void* out;         // [N][H/2][W/2][COUT]
  int N, H;
  int lgb;           // convT row sweeps: log2 of the row bands per image (0: whole images)
};

#ifdef SPECENH_CR_STATS  // development build (tools/cr_stats.py): per-wave clocks of a step's segments
__device__ unsigned long long cr_stats[1024 * 8 * 8];
struct CRClock {
  long long last = 0, seg[6] = {0, 0, 0, 0, 0, 0}, n = 0;
  // SEG (conv_rows_pool_kernel): 0 pool + store head, 1 DMA issue, 2 fragment reads until the
  // first MFMA can issue, 3 MFMA block, 4 vmcnt wait, 5 barrier wait; -1 starts the clock.
  // (enc2_rows_kernel): 0 pool + store head (schedule 1: the storing waves' tile store), 1 DMA
  // issue, 2 conv1 (schedule 1: with the pool), 3 conv2, 4 vmcnt wait, 5 barrier
  template <int SEG>
  __device__ __forceinline__ void mark() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const long long t = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SEG >= 0) seg[SEG] += t - last;
    if constexpr (SEG == 5) ++n;
    last = t;
  }
  __device__ void flush(int wv) {
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 1024) {
      unsigned long long* p = cr_stats + (blockIdx.x * 8 + wv) * 8;
#pragma unroll
      for (int i = 0; i < 6; ++i) p[i] = seg[i];
      p[6] = n;
      p[7] = 0;
    }
  }
};
#define CR_MARK(SEG) clk.mark<SEG>()
#else
#define CR_MARK(SEG) ((void)0)
#endif

// K (CIN = 32 only): the kernel size, 5 (the reference model) or 3 (hyperparam_scan.py's
// k = 3 model): K^2 resident tap fragments, K B fragments per input row, output rows
// r + K/2 - ky; the accumulator ring of 6 rows and the pooling lag are the same.
//
// SCHED: the step's schedule. Every wave runs the same program and all eight meet at one
// barrier per step, so whatever a wave does with the matrix pipe empty, its SIMD partner
// (wave w + 4) does at the same moment.
//  0 (variant CONV_ROWS_SCHED=0; the default until round 7, kept as the A/B and bitwise
//    partner): after the barrier every wave pools and stores pair s - 2, the DMA waves issue
//    the rows of step s + LEAD, all B fragments of step s are read, and only when they have
//    landed do the MFMAs start; then vmcnt(1) / vmcnt(0) — on waves 4-7 a wait for their own
//    pooled store — and the barrier.
//  1 (CIN = 32, K = 5, 256-VGPR build): the fragments of step s + PF are read during step
//    s into a second register buffer (their rows were waited for at the end of step s - 1
//    and their ring slots are refilled from step s + 2 on), so the MFMAs start right after
//    the barrier; the MFMAs into the four accumulators that were NOT just pooled go first and
//    the pool, pack and store run in their shadow (each accumulator keeps its (j, kx, ky)
//    order: bitwise equal to 0); the store's address advances by scalar adds; and only the
//    DMA waves wait on vmcnt, for the DMA they need, by the ledger of convt_rows_kernel;
//    and the counters, addresses and branch flags of step s + 1 are computed under step s's
//    MFMAs, so a step opens with a flag test instead of ~35 scalar instructions.
//    Unrolled by 6: accumulator slots (s mod 3) and fragment buffer (s mod 2) are
//    compile-time. 252 VGPRs, no scratch (schedule 0: 180).
//    conv3 + pool at 2048 shots: 0.141 ms against 0.159 ms (profiles/conv3_sched_ab.txt);
//    where the clocks of a step go in either schedule: profiles/conv3_phase_clocks.txt.
// Only <32, 64, 32, 5> is launched with schedule 1. CIN = 16 cannot read a step ahead as it
// stands: its F fragment pairs row r + 1, a row of step s + 2 when read in step s, which
// has not been waited for then. <32, 32, 64> (K = 5: a 256-VGPR build like the flagship;
// K = 3: 94 of 128 VGPRs) would compile, but neither is on the bench's path and neither has
// been timed with it, so both keep the step they were measured with.
template <typename T, int CIN, int COUT, int W, int K = 5, int SCHED = 0>
__global__ __launch_bounds__((RC<CIN, COUT, W, K>::THREADS))
__attribute__((amdgpu_waves_per_eu(RC<CIN, COUT, W, K>::WPE)))
void conv_rows_pool_kernel(CRArgs a) {
  static_assert(SCHED == 0 || (SCHED == 1 && CIN == 32), "schedule");
  using C = RC<CIN, COUT, W, K>;
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int wx = wv % C::NWIN, nb = wv / C::NWIN;
  const int x0 = 16 * wx;
  const int H = a.H, SPI = H / 2 + 1;  // steps per image: rows (2q, 2q + 1), q = 0 .. H/2
  const int G = gridDim.x;
  const int nimg = ((int)a.N - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI + 1;  // + 1: the last pair is stored one step after its rows

  {
    uint4* z = reinterpret_cast<uint4*>(ring);
    for (int e = tid; e < C::LDS / 16; e += C::THREADS) z[e] = uint4{0u, 0u, 0u, 0u};
  }

  // ---- resident weights: A operand, lane (m, kg) = output channel 16 nb + m, K 8 kg .. ----
  uint4 wf[C::NW];
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
    const int co = 16 * nb + m;
    auto tap = [&](int ky, int kx, int c8) {
      return *reinterpret_cast<const uint4*>(Wg + ((co * K + ky) * K + kx) * CIN + c8);
    };
    if constexpr (CIN == 32) {
#pragma unroll
      for (int t = 0; t < K * K; ++t) wf[t] = tap(t / K, t % K, 8 * kg);
    } else {
      const int hi = kg >> 1, c8 = 8 * (kg & 1);
#pragma unroll
      for (int ky = 0; ky < 5; ++ky) {
        wf[ky] = tap(ky, hi, c8);          // columns (0, 1)
        wf[5 + ky] = tap(ky, 2 + hi, c8);  // columns (2, 3)
      }
      wf[10] = tap(hi, 4, c8);             // F: (w[0][4], w[1][4])
      wf[11] = tap(2 + hi, 4, c8);         //    (w[2][4], w[3][4])
      wf[12] = hi ? uint4{0u, 0u, 0u, 0u} : tap(4, 4, c8);  // (w[4][4], 0)
    }
  }
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};

  // ---- this lane's B-fragment byte offsets within a ring row ----
  int boff[CIN == 32 ? K : 1];
  int foff = 0, foffw = 0, fo0 = 0;  // CIN = 16: F fragment (next row in the next slot /
                                     // wrapped), and its offset within one row
  if constexpr (CIN == 32) {
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ps = x0 + m + kx + 2 - K / 2;  // stored pixel (x + 2)
      boff[kx] = ps * 64 + 16 * (kg ^ ((ps >> 1) & 3));
    }
  } else {
    boff[0] = (x0 + m + (kg >> 1)) * 32 + 16 * (kg & 1);  // columns (0, 1); (2, 3) at + 64
    const int fo = (x0 + m + 4) * 32 + 16 * (kg & 1);
    fo0 = fo;
    foff = fo + (kg >> 1) * C::ROWB;
    foffw = fo - (kg >> 1) * 7 * C::ROWB;  // row r in slot 7: row r + 1 in slot 0
  }

  // ---- row DMA: waves 0 .. DMA_WAVES - 1, wave w moves part w % WPR of row w / WPR ----
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const bool dma_wave = wv < C::DMA_WAVES;
  int dsrc = 0, ddst = 0;
  if (dma_wave) {
    const int c = (wv % C::WPR) * 64 + lane;  // chunk of the row
    const int ps = 2 + c / C::CPP, gs = c % C::CPP;
    const int g = CIN == 32 ? (gs ^ ((ps >> 1) & 3)) : gs;
    dsrc = (ps - 2) * CIN + 8 * g;  // element offset within the image row
    ddst = 2 * C::PIX + (wv % C::WPR) * 1024;
  }
  // rows of global step s: image (s / SPI) of this workgroup, rows 2q, 2q + 1 (q = s % SPI)
  // rows of global step s = il SPI + q (the caller keeps (il, q) as scalar counters: a
  // run-time division per use cost ~25 SALU and a VALU reciprocal, three per step)
  auto stage_at = [&](int s, int il, int q) -> bool {  // whether this wave issued an LDS-DMA
    if (!dma_wave) return false;
    const int r = 2 * q + wv / C::WPR;
    unsigned char* dst = ring + ((2 * s + wv / C::WPR) & 7) * C::ROWB + ddst;
    if (s < S && il < nimg && r < H) {
      const long long n = (long long)blockIdx.x + (long long)il * G;
      lds_dma16_s(X + ((n * H + r) * W) * CIN, 2u * dsrc, dst);
      return true;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return false;
  };
  auto stage = [&](int s) { return stage_at(s, s / SPI, s - (s / SPI) * SPI); };  // (prologue)
  __syncthreads();  // ring zeroed
  stage(0);
  stage(1);
  stage(2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();

  f32x4 acc[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = bias;
  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int PW = W / 2, PHh = H / 2;

  // (image, step in image) of steps s - 2 (pool), s (conv), s + 3 (DMA), advanced per step
  int ilA = -1, qA = SPI - 2, ilC = 0, qC = 0, ilS = 3 / SPI, qS = 3 - (3 / SPI) * SPI;
  auto adv = [&](int& il, int& q) {
    if (++q == SPI) { q = 0; ++il; }
  };
#ifdef SPECENH_CR_STATS
  CRClock clk;
#endif
  if constexpr (SCHED == 1) {
    // ---- schedule 1 (header comment): fragments one step ahead, head under the MFMAs ----
    static_assert(C::PF == 1, "two fragment buffers");
    uint4 bf[2][2][K];
    // row j of step t's input rows -> fragment buffer P (rows 2t, 2t + 1 sit in two
    // consecutive ring slots, the first one even: never wrapped)
    auto frags = [&](auto pc, auto jc, const int t) {
      constexpr int P = decltype(pc)::value, j = decltype(jc)::value;
      const unsigned char* rb = ring + (((2 * t) & 7) + j) * C::ROWB;
#pragma unroll
      for (int kx = 0; kx < K; ++kx) bf[P][j][kx] = *reinterpret_cast<const uint4*>(rb + boff[kx]);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    frags(I0{}, I0{}, 0);
    frags(I0{}, I1{}, 0);
    resident_loads_landed();
    // the pooled pair's store: wave-uniform row address (scalar adds per step) + the lane's
    // constant byte offset
    constexpr long long ROWO = (long long)(W / 2) * COUT * (long long)sizeof(T);
    const unsigned ovo = (unsigned)((((x0 + m) / 2) * COUT + 16 * nb + 4 * kg) * (int)sizeof(T));
    unsigned char* ob = reinterpret_cast<unsigned char*>(a.out) +
                        (((long long)blockIdx.x - G) * PHh + qA) * ROWO;  // pair (ilA, qA)
    const long long ojump = (long long)(G - 1) * PHh * ROWO;  // (il, SPI - 1) -> (il + 1, 0)
    // the DMA's source, likewise: this wave's row of step s + LEAD (rows 2 qS, 2 qS + 1 of
    // image ilS), advanced by two rows per step and by the rest of the grid's images at a wrap
    constexpr long long ROWX = (long long)W * CIN * (long long)sizeof(T);
    const unsigned char* xs = reinterpret_cast<const unsigned char*>(a.x) +
        (((long long)blockIdx.x + (long long)ilS * G) * H + 2 * qS + wv / C::WPR) * ROWX;
    const long long xjump = (long long)(G - 1) * H * ROWX;  // (il, SPI - 1) -> (il + 1, 0)
    int vmn = 0;           // this wave's vector-memory ops issued in the loop (DMAs, stores)
    int mk0 = -1, mk1 = -1;  // vmn right after the DMA of steps s - 1 / s (-1: none)
    // what the step's branches ask, from the counters: 1 the step has input rows, 2 pair s - 2
    // is an output row, 4 the rows of step s + LEAD are inside an image (H is even: both rows)
    // (a < b as the difference's sign bit: a compare turned into an integer went through a
    // VGPR, which the scalar asm operand below cannot take)
    auto lt = [](int x, int y) -> unsigned { return (unsigned)(x - y) >> 31; };
    // (values that a run-time division made on the VALU, into scalar registers for good)
    const int nimgs = __builtin_amdgcn_readfirstlane(nimg);
    ilS = __builtin_amdgcn_readfirstlane(ilS);
    qS = __builtin_amdgcn_readfirstlane(qS);
    auto flags = [&]() -> unsigned {
      return (lt(ilC, nimgs) & lt(2 * qC, H)) | ((lt(-1, ilA) & lt(ilA, nimgs) & lt(qA, PHh)) << 1) |
             ((lt(ilS, nimgs) & lt(2 * qS, H)) << 2);
    };
    unsigned fl = __builtin_amdgcn_readfirstlane(flags());
    // The counters, addresses and flags of step s + 1, computed under step s's MFMAs: after
    // the barrier a step starts with a branch on a flag, not with ~35 scalar instructions
    // that both waves of a SIMD run with the matrix pipe empty. The empty asm pins the
    // results where it stands (the compiler otherwise sinks them to their uses).
    auto next = [&]() {
      if (++qA == SPI) { qA = 0; ++ilA; ob += ojump; } else { ob += ROWO; }
      adv(ilC, qC);
      if (++qS == SPI) { qS = 0; ++ilS; xs += xjump; } else { xs += 2 * ROWX; }
      fl = __builtin_amdgcn_readfirstlane(flags());
      asm volatile("" : "+s"(fl));
    };
    auto step1 = [&](auto ic, const int s) {
      constexpr int I = decltype(ic)::value % 3, P = decltype(ic)::value & 1;
      auto slot = [](int d) { return (2 * I + d + 12) % 6; };
      using PN = std::integral_constant<int, P ^ 1>;
      // (1) rows of step s + LEAD into the ring
      mk1 = -1;
      if (dma_wave) {
        unsigned char* dst = ring + ((2 * (s + C::LEAD) + wv / C::WPR) & 7) * C::ROWB + ddst;
        if (fl & 4u) {
          lds_dma16_s(xs, 2u * dsrc, dst);
          mk1 = ++vmn;
        } else {
          *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
        }
      }
      CR_MARK(1);
      f32x4& r0 = acc[slot(-4)];
      f32x4& r1 = acc[slot(-3)];
      const bool pst = (fl & 2u) != 0;  // pair s - 2 is an output row
      // pair s - 2 (output rows 2q - 4, 2q - 3) is complete: pool, pack, reset
      auto pool = [&]() {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(max_pair(fmaxf(r0[i], r1[i])), 0.f);
        r0 = bias;
        r1 = bias;
        return uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])};
      };
      // lanes m, m ^ 1 hold the same pooled values: both store them (no exec-mask branch)
      auto store = [&](const uint2 pk) {
        if (pst) {
          gstore8_s(ob, ovo, pk);
          ++vmn;
        }
      };
      auto mm = [&](int j, int kx, int ky) {
        f32x4& ac = acc[slot(j + K / 2 - ky)];
        ac = mfma16x16x32<T>(wf[ky * K + kx], bf[P][j][kx], ac);
      };
      if (fl & 1u) {
        // first the row-0 MFMAs into the accumulators that are still summing (d <= 1); the
        // pool and the first half of the next step's fragment reads go in their shadow
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
            if (K / 2 - ky <= 1) mm(0, kx, ky);
        const uint2 pk = pool();
        frags(PN{}, I0{}, s + 1);
        store(pk);
        next();
        // the other half of the reads ahead of the remaining MFMAs (the compiler barrier keeps
        // them from being merged with the bubble path's reads below the MFMAs)
        frags(PN{}, I1{}, s + 1);
        asm volatile("" ::: "memory");
        // then, per tap column, the row-0 MFMAs into the two reset accumulators with the
        // row-1 MFMAs into the others between them, and last the row-1 MFMAs into the reset ones
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
            if (K / 2 - ky > 1) mm(0, kx, ky);
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
            if (1 + K / 2 - ky <= 1) mm(1, kx, ky);
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int ky = 0; ky < K; ++ky)
            if (1 + K / 2 - ky > 1) mm(1, kx, ky);
      } else {  // the bubble between images (and the steps past the last rows)
        store(pool());
        next();
        frags(PN{}, I0{}, s + 1);
        frags(PN{}, I1{}, s + 1);
      }
      CR_MARK(3);
      // (2) rows of step s + LEAD - 1 (DMA issued at step s - 1) have landed: the DMA waves
      // wait for that DMA alone, the ops issued after it (up to two stores and this step's DMA)
      // counted out; waves 4-7 never wait on vmcnt
      if (mk0 >= 0) {
        const int younger = vmn - mk0;
        if (younger >= 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (younger == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      mk0 = mk1;
      CR_MARK(4);
      lds_barrier();
      CR_MARK(5);
    };
    CR_MARK(-1);
    int s = 0;
    for (; s + 6 <= S; s += 6) {
      step1(std::integral_constant<int, 0>{}, s);
      step1(std::integral_constant<int, 1>{}, s + 1);
      step1(std::integral_constant<int, 2>{}, s + 2);
      step1(std::integral_constant<int, 3>{}, s + 3);
      step1(std::integral_constant<int, 4>{}, s + 4);
      step1(std::integral_constant<int, 5>{}, s + 5);
    }
    if (s < S) step1(std::integral_constant<int, 0>{}, s);
    if (s + 1 < S) step1(std::integral_constant<int, 1>{}, s + 1);
    if (s + 2 < S) step1(std::integral_constant<int, 2>{}, s + 2);
    if (s + 3 < S) step1(std::integral_constant<int, 3>{}, s + 3);
    if (s + 4 < S) step1(std::integral_constant<int, 4>{}, s + 4);
#ifdef SPECENH_CR_STATS
    clk.flush(wv);
#endif
    return;
  }
  // step s with I = s % 3 compile-time (the accumulator ring: output row 2q + d -> slot
  // (2 I + d) mod 6)
  auto step = [&](auto ic, const int s) {
    constexpr int I = decltype(ic)::value;
    auto slot = [](int d) { return (2 * I + d + 12) % 6; };
    // (1) pair s - 2 (output rows 2q - 4, 2q - 3) is complete: pool, store, reset
    {
      f32x4& r0 = acc[slot(-4)];
      f32x4& r1 = acc[slot(-3)];
      {
        const int il = ilA, q = qA;  // pair s - 2
        if (il >= 0 && il < nimg && q < PHh) {
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(max_pair(fmaxf(r0[i], r1[i])), 0.f);
          // lanes m, m ^ 1 hold the same pooled values: both store them (no exec-mask branch)
          const long long n = (long long)blockIdx.x + (long long)il * G;
          const long long o = ((n * PHh + q) * PW + (x0 + m) / 2) * COUT + 16 * nb + 4 * kg;
          *reinterpret_cast<uint2*>(O + o) = uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])};
        }
      }
      r0 = bias;
      r1 = bias;
    }
    CR_MARK(0);
    // (2) rows of step s + 3 into the ring
    const bool issued = stage_at(s + C::LEAD, ilS, qS);
    CR_MARK(1);
    // (3) this step's input rows
    const int il = ilC, q = qC;
    if (il < nimg && 2 * q < H) {
      // every B fragment of the step first (one LDS latency per step, not one per row or
      // tap column: sched_barrier keeps the compiler from sinking the reads to their MFMAs)
      constexpr int NB = CIN == 32 ? K : 3;
      uint4 bf[2][NB];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int rs = (2 * s + j) & 7;
        const unsigned char* rb = ring + rs * C::ROWB;
        if constexpr (CIN == 32) {
#pragma unroll
          for (int kx = 0; kx < K; ++kx) bf[j][kx] = *reinterpret_cast<const uint4*>(rb + boff[kx]);
        } else {
          bf[j][0] = *reinterpret_cast<const uint4*>(rb + boff[0]);
          bf[j][1] = *reinterpret_cast<const uint4*>(rb + boff[0] + 64);
          bf[j][2] = *reinterpret_cast<const uint4*>(rb + (rs == 7 ? foffw : foff));
        }
      }
      uint4 bT = uint4{0u, 0u, 0u, 0u};
      if constexpr (CIN == 16) {
        if (q == 0) {
          // F(-1) = (row -1, row 0): output row 1 gets w[1][4] x row 0. Row -1 is zero
          // padding (not read: its ring slot is being refilled by this step's stage)
          bT = *reinterpret_cast<const uint4*>(ring + ((2 * s) & 7) * C::ROWB + fo0);
          if (kg < 2) bT = uint4{0u, 0u, 0u, 0u};
        }
      }
      CR_MARK(2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (CIN == 32) {
#pragma unroll
          for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int ky = 0; ky < K; ++ky) {
              f32x4& ac = acc[slot(j + K / 2 - ky)];
              ac = mfma16x16x32<T>(wf[ky * K + kx], bf[j][kx], ac);
            }
        } else {
          // consecutive MFMAs into different accumulators (no back-to-back dependency)
#pragma unroll
          for (int ky = 0; ky < 5; ++ky) {
            f32x4& ac = acc[slot(j + 2 - ky)];
            ac = mfma16x16x32<T>(wf[ky], bf[j][0], ac);
          }
#pragma unroll
          for (int ky = 0; ky < 5; ++ky) {
            f32x4& ac = acc[slot(j + 2 - ky)];
            ac = mfma16x16x32<T>(wf[5 + ky], bf[j][1], ac);
          }
          acc[slot(j + 2)] = mfma16x16x32<T>(wf[10], bf[j][2], acc[slot(j + 2)]);
          acc[slot(j)] = mfma16x16x32<T>(wf[11], bf[j][2], acc[slot(j)]);
          acc[slot(j - 2)] = mfma16x16x32<T>(wf[12], bf[j][2], acc[slot(j - 2)]);
          if (j == 0 && q == 0) acc[slot(1)] = mfma16x16x32<T>(wf[10], bT, acc[slot(1)]);
        }
      }
    }
    // (4) rows of step s + 2 (DMA issued at step s - 1) have landed; this step's stores are
    // older than its DMA and complete too
    CR_MARK(3);
    if (issued) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    CR_MARK(4);
    adv(ilA, qA);
    adv(ilC, qC);
    adv(ilS, qS);
    lds_barrier();
    CR_MARK(5);
  };
  CR_MARK(-1);
  int s = 0;
  for (; s + 3 <= S; s += 3) {
    step(std::integral_constant<int, 0>{}, s);
    step(std::integral_constant<int, 1>{}, s + 1);
    step(std::integral_constant<int, 2>{}, s + 2);
  }
  if (s < S) step(std::integral_constant<int, 0>{}, s);
  if (s + 1 < S) step(std::integral_constant<int, 1>{}, s + 1);
#ifdef SPECENH_CR_STATS
  clk.flush(wv);
#endif
}

template <typename T, int CIN, int COUT, int W, int K = 5, int SCHED = 0>
hipError_t launch_rows(const CRArgs& a, hipStream_t st) {
  using C = RC<CIN, COUT, W, K>;
  const void* k = reinterpret_cast<const void*>(&conv_rows_pool_kernel<T, CIN, COUT, W, K, SCHED>);
  static ResidentSlots site;
  long long slots = 0;
  const hipError_t e = resident_slots(site, k, C::THREADS, C::LDS, &slots);
  if (e != hipSuccess) return e;
  const long long grid = std::min<long long>(a.N, slots);
  SPECENH_LAUNCH((conv_rows_pool_kernel<T, CIN, COUT, W, K, SCHED>), dim3((unsigned)grid),
                 dim3(C::THREADS), C::LDS, st, a);
  return hipGetLastError();
}

// ============================================================================ convT rows
// Conv2DTranspose(CO, 5, strides=2, relu, same) on 64-channel inputs as a row sweep
// (VAE/manual_scan_3layers.py:196-197: the decoder's 64 -> 64 at 16 x 16 -> 32 x 32 and,
// outside the fused decoder, 64 -> 32 at 32 x 32 -> 64 x 64). conv_patch_kernel runs the
// four output phases as dense convs over 16 x 16 tiles (0.20 of the MFMA peak). Here, as in
// decoder3's producer waves (decoder_tail.hip), input position row s yields output rows
// 2s, 2s + 1: for each of the 9 neighbourhood offsets (dy, dx) one B fragment pair (input
// row s + dy shifted by dx, 16 positions x 64 channels, two K = 32 halves) feeds every
// phase that has the tap — 50 MFMAs from 18 LDS reads per (row, 16 positions, 16 output
// channels). Output phase (py, px) of position (s, x) is pixel (2s + py, 2x + px), its tap
// (ky, kx) = (2 dy + 3 - py, 2 dx + 3 - px) when inside the 5 x 5 kernel (pad 3 of the
// dilated-input conv): 4 / 6 / 6 / 9 taps, exactly the 25 useful ones.
//  * wave (window wx, channel block nb) holds its 50 tap fragments (A operand) in registers
//    for the launch; the four phase accumulators start at the bias.
//  * the input rows are one stream per persistent workgroup: position p = il (H + 1) + 1 + r
//    holds row r of the workgroup's image il, position il (H + 1) the zero row between
//    images, so step g (image g / (H + 1), row s = g % (H + 1), s = H a bubble) reads
//    positions g .. g + 2 and the ring refill is one position per step (LDS-DMA, 3 steps
//    ahead, 8-row ring).
//  * the packed outputs of step g are stored at the start of step g + 1, ahead of that
//    step's DMA, so the end-of-step vmcnt wait (everything but that DMA) never waits on a
//    store younger than the DMA it needs.
// Input pixels are 128 B with their 16-byte groups swizzled, g ^ (p & 7) (decoder3's x1_off:
// conflict-free fragment reads).
template <int CO, int W>
struct TC {
  static constexpr int CI = 64;
  static constexpr int NWIN = W / 16, NNB = CO / 16;
  static constexpr int WAVES = NWIN * NNB;
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int ROWB = (W + 2) * CI * 2;  // one zero position each side
  static constexpr int RING = 8;
  static constexpr int LDS = RING * ROWB;
  static constexpr int DMA_WAVES = W * CI * 2 / 1024;  // one 1-KB DMA per wave and row
  static_assert(WAVES == 4 && DMA_WAVES <= WAVES, "shape");
};

__device__ __forceinline__ constexpr int tky(int py, int dy) { return 2 * dy + 3 - py; }
__device__ __forceinline__ constexpr bool ttap(int ph, int dy, int dx) {
  return tky(ph >> 1, dy) >= 0 && tky(ph >> 1, dy) < 5 && tky(ph & 1, dx) >= 0 &&
         tky(ph & 1, dx) < 5;
}

// bias + ReLU of four fp32 accumulators -> four T in 8 bytes. ReLU commutes with the monotone
// rounding, so it runs on the packed 16-bit pairs: v_pk_max_f16 for fp16; for bf16 each half's
// sign is spread over the half by a packed arithmetic shift and cleared with one bitfield select
// (-0 -> +0 as max(x, 0) gives it). fmaxf on the fp32 accumulators cost 32 VALU per 16 values
// (the max and a NaN-quieting max per element), these 4-6.
template <typename T>
__device__ __forceinline__ uint32_t relu2(uint32_t p) {
  if constexpr (__is_same(T, _Float16)) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 z = h2{(_Float16)0.f, (_Float16)0.f};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(h2, p), z));
  } else {
    typedef short s2 __attribute__((ext_vector_type(2)));
    const uint32_t neg = __builtin_bit_cast(uint32_t, __builtin_bit_cast(s2, p) >> (short)15);
    return p & ~neg;
  }
}
template <typename T>
__device__ __forceinline__ uint2 relu_pack4(const f32x4& v) {
  return uint2{relu2<T>(pack2_cvt<T>(v[0], v[1])), relu2<T>(pack2_cvt<T>(v[2], v[3]))};
}

// LEAD: ring refills in flight beyond the one a step waits for. Step g needs positions
// g + 1 .. g + 3 after its barrier, so it waits for the DMA of position g + 3 only, issued LEAD
// steps earlier; the wave's ledger of its vector-memory ops (LDS-DMAs, and the output stores,
// which vmcnt counts too on gfx9) turns that into the count of younger ops. Round 3 waited
// with vmcnt(1) for everything but the DMA just issued, i.e. for the previous step's DMA and
// this step's own stores.
template <typename T, int CO, int W, int LEAD>
__global__ __launch_bounds__((TC<CO, W>::THREADS)) __attribute__((amdgpu_waves_per_eu(2)))
void convt_rows_kernel(CRArgs a) {
  static_assert(LEAD >= 1 && LEAD <= 4, "8-row ring: positions g .. g + 3 + LEAD live");
  using C = TC<CO, W>;
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int wx = wv % C::NWIN, nb = wv / C::NWIN;
  // the stream's units: whole images (lgb = 0) or row bands of HB rows (small batches)
  const int H = a.H, lgb = a.lgb, HB = H >> lgb, bmask = (1 << lgb) - 1;
  const int SPI = HB + (lgb ? 2 : 1);
  const int G = gridDim.x;
  const int nimg = (((int)a.N << lgb) - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  {
    uint4* z = reinterpret_cast<uint4*>(ring);
    for (int e = tid; e < C::LDS / 16; e += C::THREADS) z[e] = uint4{0u, 0u, 0u, 0u};
  }
  // tap fragments [phase][(dy, dx) taps][K half]
  uint4 wf[50];
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
    int u = 0;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (!ttap(ph, dy, dx)) continue;
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
            wf[u++] = *reinterpret_cast<const uint4*>(
                Wg + (((16 * nb + m) * 5 + tky(ph >> 1, dy)) * 5 + tky(ph & 1, dx)) * 64 +
                32 * kh + 8 * kg);
        }
  }
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};
  resident_loads_landed();
  int xo[3];  // byte offset of pixel 16 wx + m + dx (stored + 1), group kg, in a ring row
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    const int ps = 16 * wx + m + dx + 1;
    xo[dx + 1] = ps * 128 + 16 * (kg ^ (ps & 7));
  }
  // ring refill: wave w < DMA_WAVES moves chunks 64 w .. 64 w + 63 of a row
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const bool dma_wave = wv < C::DMA_WAVES;
  int dsrc = 0;
  if (dma_wave) {
    const int c = 64 * wv + lane;
    const int ps = 1 + c / 8, gs = c & 7;
    dsrc = (ps - 1) * 64 + 8 * (gs ^ (ps & 7));
  }
  // stream position p = il SPI + q -> ring slot p & 7: row r0 + q - 1 of the workgroup's unit
  // il (unit v = blockIdx.x + il G: image v >> lgb, first row r0 = (v & bmask) HB); rows
  // outside the image are the zero rows (one between whole images, two between bands)
  auto stage_at = [&](int p, int il, int q) -> bool {
    if (!dma_wave) return false;
    unsigned char* dst = ring + (p & 7) * C::ROWB + 128 + 1024 * wv;
    const int v = (int)blockIdx.x + il * G;
    const int r = (v & bmask) * HB + q - 1;
    if (il < nimg && r >= 0 && r < H) {
      const long long n = (long long)(v >> lgb);
      lds_dma16_s(X + ((n * H + r) * W) * 64, 2u * dsrc, dst);
      return true;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return false;
  };
  auto stage = [&](int p) -> bool {  // (prologue)
    const int il = p / SPI;
    return stage_at(p, il, p - il * SPI);
  };
  __syncthreads();  // ring zeroed
#pragma unroll
  for (int p = 0; p < 3 + LEAD; ++p) stage(p);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();

  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int OW = 2 * W;
  uint2 pk[4];
  long long po = 0;   // element offset of the held outputs' (2s, 2x) pixel
  bool held = false;  // (wave-uniform, as convt_rows_pw_kernel's)
  int vmn = 0;        // this wave's vector-memory ops issued in the loop
  int mk[LEAD + 1];   // vmn right after the DMA of position g + 3 + i (-1: none in flight)
#pragma unroll
  for (int i = 0; i <= LEAD; ++i) mk[i] = -1;
  auto store_held = [&]() {
    if (held) {
#pragma unroll
      for (int ph = 0; ph < 4; ++ph)
        gstore8(O + po + ((ph >> 1) * OW + (ph & 1)) * CO, pk[ph]);
      vmn += 4;
    }
  };
  // scalar counters (image, step in image) of step g and of its refill position g + 3 + LEAD
  int il = 0, s = 0;
  int ilp = (3 + LEAD) / SPI, sp = 3 + LEAD - ilp * SPI;
  for (int g = 0; g < S; ++g) {
    store_held();
    held = false;
    mk[LEAD] = stage_at(g + 3 + LEAD, ilp, sp) ? ++vmn : -1;
    if (s < HB) {
      f32x4 acc[4] = {bias, bias, bias, bias};
      int u0[4] = {0, 8, 20, 32};
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const unsigned char* src = ring + ((g + 1 + dy) & 7) * C::ROWB;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          // K half 1 (groups kg + 4) sits at the half-0 offset ^ 64 bytes (swizzle bit 2)
          const uint4 b0 = *reinterpret_cast<const uint4*>(src + xo[dx + 1]);
          const uint4 b1 = *reinterpret_cast<const uint4*>(src + (xo[dx + 1] ^ 64));
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) acc[ph] = mfma16x16x32<T>(wf[u0[ph]], b0, acc[ph]);
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) {
              acc[ph] = mfma16x16x32<T>(wf[u0[ph] + 1], b1, acc[ph]);
              u0[ph] += 2;
            }
        }
      }
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) pk[ph] = relu_pack4<T>(acc[ph]);
      const int v = (int)blockIdx.x + il * G;
      const long long n = (long long)(v >> lgb);
      po = ((n * 2 * H + 2 * ((v & bmask) * HB + s)) * OW + 2 * (16 * wx + m)) * CO + 16 * nb + 4 * kg;
      held = true;
    }
    if (mk[0] >= 0) wait_vmcnt_ss<15>(vmn - mk[0]);  // position g + 3 has landed
    lds_barrier();
#pragma unroll
    for (int i = 0; i < LEAD; ++i) mk[i] = mk[i + 1];
    if (++s == SPI) { s = 0; ++il; }
    if (++sp == SPI) { sp = 0; ++ilp; }
  }
  store_held();
}

// convt_rows_pw_store8_kernel (variant CONVT_STORE8; the default of rounds 4-6, kept as the A/B
// and bitwise partner of convt_rows_pw_kernel below): convT1 (CO = 64 on 16-position rows),
// every wave with its OWN input ring and 8-byte stores. The four waves of
// convt_rows_kernel<T, 64, 16> (one per 16-channel block) all read the whole input row, so
// they shared one ring filled by two of them and met at a workgroup barrier
// every step. Here each wave LDS-DMAs the row (2 x 1 KB) into its own 8-row ring (18 KB; 72 KB
// per workgroup, two workgroups per CU) and waits only for its own refill: no barrier in the
// step loop, the two waves of a SIMD drift freely against each other. The input is read from
// L2 four times instead of once (it is 32 KB per image against 128 KB of output).
template <typename T, int LEAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void convt_rows_pw_store8_kernel(CRArgs a) {
  static_assert(LEAD >= 1 && LEAD <= 4, "8-row ring: positions g .. g + 3 + LEAD live");
  using C = TC<64, 16>;
  constexpr int CO = 64, W = 16;
  constexpr int WR = C::RING * C::ROWB;  // bytes per wave ring
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_pw[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int nb = wv;
  unsigned char* const ring = lds_pw + wv * WR;
  // units: whole images or row bands, as convt_rows_kernel's
  const int H = a.H, lgb = a.lgb, HB = H >> lgb, bmask = (1 << lgb) - 1;
  const int SPI = HB + (lgb ? 2 : 1);
  const int G = gridDim.x;
  const int nimg = (((int)a.N << lgb) - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  for (int e = lane; e < WR / 16; e += 64) reinterpret_cast<uint4*>(ring)[e] = uint4{0u, 0u, 0u, 0u};
  // the zero fill's ds_writes and the prologue's LDS-DMA writes into the same ring take
  // different paths with no mutual ordering: the writes complete before any DMA is issued
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  uint4 wf[50];  // tap fragments [phase][(dy, dx) taps][K half]
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
    int u = 0;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (!ttap(ph, dy, dx)) continue;
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
            wf[u++] = *reinterpret_cast<const uint4*>(
                Wg + (((16 * nb + m) * 5 + tky(ph >> 1, dy)) * 5 + tky(ph & 1, dx)) * 64 +
                32 * kh + 8 * kg);
        }
  }
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};
  resident_loads_landed();
  int xo[3];  // byte offset of pixel m + dx (stored + 1), group kg, in a ring row
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    const int ps = m + dx + 1;
    xo[dx + 1] = ps * 128 + 16 * (kg ^ (ps & 7));
  }
  // refill: 16-byte chunks c = lane and 64 + lane of a row (pixel 1 + c / 8, swizzled group)
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  int dsrc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 64 * h + lane;
    const int ps = 1 + c / 8, gs = c & 7;
    dsrc[h] = (ps - 1) * 64 + 8 * (gs ^ (ps & 7));
  }
  // stream position p = il SPI + q -> ring slot p & 7 (row r0 + q - 1 of unit il, as
  // convt_rows_kernel's); returns the DMAs issued
  auto stage_at = [&](int p, int il, int q) -> int {
    unsigned char* dst = ring + (p & 7) * C::ROWB + 128;
    const int v = (int)blockIdx.x + il * G;
    const int r = (v & bmask) * HB + q - 1;
    if (il < nimg && r >= 0 && r < H) {
      const long long n = (long long)(v >> lgb);
      const T* src = X + ((n * H + r) * W) * 64;
      lds_dma16_s(src, 2u * dsrc[0], dst);
      lds_dma16_s(src, 2u * dsrc[1], dst + 1024);
      return 2;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    *reinterpret_cast<uint4*>(dst + 1024 + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return 0;
  };
#pragma unroll
  for (int p = 0; p < 3 + LEAD; ++p) {
    const int il = p / SPI;
    stage_at(p, il, p - il * SPI);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  constexpr int OW = 2 * W;
  uint2 pk[4];
  long long po = 0;    // element offset of the held outputs' (2s, 2x) pixel
  bool held = false;   // (wave-uniform: a per-lane "po >= 0" test had made the ledger below
                       // per-lane VGPRs, the stores an exec-masked region and the wait a ladder)
  int vmn = 0;         // this wave's vector-memory ops issued in the loop
  int mk[LEAD + 1];    // vmn right after the DMAs of position g + 3 + i (-1: none in flight)
#pragma unroll
  for (int i = 0; i <= LEAD; ++i) mk[i] = -1;
  auto store_held = [&]() {
    if (held) {
#pragma unroll
      for (int ph = 0; ph < 4; ++ph)
        gstore8(O + po + ((ph >> 1) * OW + (ph & 1)) * CO, pk[ph]);
      vmn += 4;
    }
  };
  int il = 0, s = 0;
  int ilp = (3 + LEAD) / SPI, sp = 3 + LEAD - ilp * SPI;
  for (int g = 0; g < S; ++g) {
    store_held();
    held = false;
    const int nd = stage_at(g + 3 + LEAD, ilp, sp);
    vmn += nd;
    mk[LEAD] = nd ? vmn : -1;
    if (s < HB) {
      f32x4 acc[4] = {bias, bias, bias, bias};
      int u0[4] = {0, 8, 20, 32};
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const unsigned char* src = ring + ((g + 1 + dy) & 7) * C::ROWB;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const uint4 b0 = *reinterpret_cast<const uint4*>(src + xo[dx + 1]);
          const uint4 b1 = *reinterpret_cast<const uint4*>(src + (xo[dx + 1] ^ 64));
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) acc[ph] = mfma16x16x32<T>(wf[u0[ph]], b0, acc[ph]);
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) {
              acc[ph] = mfma16x16x32<T>(wf[u0[ph] + 1], b1, acc[ph]);
              u0[ph] += 2;
            }
        }
      }
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) pk[ph] = relu_pack4<T>(acc[ph]);
      const int v = (int)blockIdx.x + il * G;
      const long long n = (long long)(v >> lgb);
      po = ((n * 2 * H + 2 * ((v & bmask) * HB + s)) * OW + 2 * m) * CO + 16 * nb + 4 * kg;
      held = true;
    }
    // this wave's refill of position g + 3 (both DMAs) has landed; LDS reads are in order
    // within a wave, so the zero-filled rows need no wait. Steady state: 3 steps of 4 stores
    // + 2 DMAs younger than it, i.e. >= 15
    if (mk[0] >= 0) wait_vmcnt_ss<15>(vmn - mk[0]);
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < LEAD; ++i) mk[i] = mk[i + 1];
    if (++s == SPI) { s = 0; ++il; }
    if (++sp == SPI) { sp = 0; ++ilp; }
  }
  store_held();
}

// convt_rows_pw_kernel (convT1's default): the step's outputs staged in LDS and stored as whole
// cache lines. The store8 kernel above wrote 8 bytes per lane: one store instruction touched 16
// lines, 32 bytes each, and every 128-byte output pixel came from four unsynchronised waves;
// with the stores taken out it ran 0.092 instead of 0.119 ms per 2048 shots. A
// step's two output rows (2 x 32 pixels x 64 channels) are ONE contiguous 8 KB of the NHWC
// output, so:
//  * after relu_pack4 a wave writes its four 8-byte pieces per lane into an 8 KB tile in LDS
//    (double-buffered: a wave may compute step g + 1 while another still stores step g). Piece
//    u = 4 nb + kg of pixel (py, p = 2 m + px) sits at byte 4096 py + 128 p + 8 (u ^ m): the 16
//    lanes of a ds_write_b64 group (one kg, m = 0 .. 15) cover all 32 banks once.
//  * after the step's barrier wave w stores bytes 2048 w .. 2048 w + 2047 of the tile with two
//    16-byte-per-lane instructions, each 1 KB contiguous (eight whole pixels). Lane l reads the
//    16-byte chunk c = l & 7 of its pixel at chunk c ^ (m >> 1) (conflict-free under the
//    ds_read_b128 lane groups) and swaps its halves when m is odd (m & 1 = (l >> 4) & 1).
//  * the barrier being there anyway, the input ring is one per workgroup, filled by waves 0
//    and 1 (convt_rows_kernel's scheme): 0.5 DMAs per wave-step instead of 2.
//  * the step loop is unrolled by the ring length, so ring slots and tile buffers are immediate
//    offsets; the tile's output offset and the refill's source row advance by scalar adds.
// The outputs of step g are still stored at the start of step g + 1, ahead of that step's DMA.
// The per-phase MFMA order is the store8 kernel's: bitwise equal.
constexpr int CT_TILE = 2 * 32 * 64 * 2;  // bytes: two output rows of 32 pixels x 64 channels
// (the tile maps are restated in tests/test_convt_stage_mapping.py)
// the lane's piece of phase (0, 0); phase (py, px) adds 4096 py + 128 px
__device__ __forceinline__ constexpr int ct_tile_write(int nb, int m, int kg) {
  return 256 * m + 8 * ((4 * nb + kg) ^ m);
}
// where the 16 bytes of tile byte L = 2048 w + 1024 j + 16 l (wave w, lane l, store j) sit
__device__ __forceinline__ constexpr int ct_tile_read(int w, int l, int j) {
  const int L = 2048 * w + 1024 * j + 16 * l, p = (L >> 7) & 31;
  return (L & ~0x70) | (((l & 7) ^ (p >> 2)) << 4);
}

template <typename T, int LEAD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void convt_rows_pw_kernel(CRArgs a) {
  static_assert(LEAD >= 1 && LEAD <= 4, "8-row ring: positions g .. g + 3 + LEAD live");
  using C = TC<64, 16>;
  constexpr int W = 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_st[];
  unsigned char* const ring = lds_st;            // 8 input rows
  unsigned char* const tile = lds_st + C::LDS;   // 2 output tiles
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int nb = wv;
  // units: whole images or row bands, as convt_rows_kernel's. Unit v = blockIdx.x + il G is
  // rows v HB .. v HB + HB - 1 of the [N H] row stream (H = HB << lgb)
  const int H = a.H, lgb = a.lgb, HB = H >> lgb, bmask = (1 << lgb) - 1;
  const int SPI = HB + (lgb ? 2 : 1);
  const int G = gridDim.x;
  const int nimg = (((int)a.N << lgb) - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  {
    uint4* z = reinterpret_cast<uint4*>(ring);
    for (int e = tid; e < C::LDS / 16; e += 256) z[e] = uint4{0u, 0u, 0u, 0u};
  }
  uint4 wf[50];  // tap fragments [phase][(dy, dx) taps][K half]
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
    int u = 0;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if (!ttap(ph, dy, dx)) continue;
#pragma unroll
          for (int kh = 0; kh < 2; ++kh)
            wf[u++] = *reinterpret_cast<const uint4*>(
                Wg + (((16 * nb + m) * 5 + tky(ph >> 1, dy)) * 5 + tky(ph & 1, dx)) * 64 +
                32 * kh + 8 * kg);
        }
  }
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};
  resident_loads_landed();
  int xo[3];  // byte offset of pixel m + dx (stored + 1), group kg, in a ring row
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    const int ps = m + dx + 1;
    xo[dx + 1] = ps * 128 + 16 * (kg ^ (ps & 7));
  }
  // per-lane tile addresses: the wave's four pieces, its two read-back chunks, their place in
  // the 8 KB of output
  unsigned char* const tw = tile + ct_tile_write(nb, m, kg);
  const unsigned char* const tr0 = tile + ct_tile_read(wv, lane, 0);
  const unsigned char* const tr1 = tile + ct_tile_read(wv, lane, 1);
  const unsigned swp = 0u - ((lane >> 4) & 1);  // all ones: swap the chunk's halves
  const unsigned vo = 2048u * wv + 16u * lane;
  // ring refill: wave w < 2 moves chunks 64 w .. 64 w + 63 of a row
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const bool dma_wave = wv < C::DMA_WAVES;
  int dsrc = 0;
  if (dma_wave) {
    const int c = 64 * wv + lane;
    const int ps = 1 + c / 8, gs = c & 7;
    dsrc = (ps - 1) * 64 + 8 * (gs ^ (ps & 7));
  }
  // stream position il SPI + q -> ring slot `slot`: row q - 1 of unit v (il-th of the
  // workgroup); rows outside the image are the zero rows
  auto stage_at = [&](int slot, int il, int v, int q) __attribute__((always_inline)) -> bool {
    if (!dma_wave) return false;
    unsigned char* dst = ring + slot * C::ROWB + 128 + 1024 * wv;
    const int r = (v & bmask) * HB + q - 1;
    if (il < nimg && r >= 0 && r < H) {
      lds_dma16_s(X + (long long)(v * HB + q - 1) * (W * 64), 2u * dsrc, dst);
      return true;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return false;
  };
  __syncthreads();  // ring zeroed
#pragma unroll
  for (int p = 0; p < 3 + LEAD; ++p) {
    const int il = p / SPI;
    stage_at(p & 7, il, (int)blockIdx.x + il * G, p - il * SPI);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();

  unsigned char* const Ob = reinterpret_cast<unsigned char*>(a.out);
  bool held = false;     // (wave-uniform) a tile waits in LDS for its stores
  unsigned hob = 0;      // its byte offset in the output (host-checked < 2^32)
  int vmn = 0;           // this wave's vector-memory ops issued in the loop
  int mk[LEAD + 1];      // vmn right after the DMA of position g + 3 + i (-1: none in flight)
#pragma unroll
  for (int i = 0; i <= LEAD; ++i) mk[i] = -1;
  // the held tile (buffer at byte tb of the tile area) -> output: two 1 KB stores per wave
  auto store_held = [&](int tb) __attribute__((always_inline)) {
    if (held) {
      uint4 v0 = *reinterpret_cast<const uint4*>(tr0 + tb);
      uint4 v1 = *reinterpret_cast<const uint4*>(tr1 + tb);
      // (halves swapped where m is odd: bit selects, no exec-masked region in the step)
      auto sel = [&](unsigned x, unsigned y) { return (x & ~swp) | (y & swp); };
      v0 = uint4{sel(v0.x, v0.z), sel(v0.y, v0.w), sel(v0.z, v0.x), sel(v0.w, v0.y)};
      v1 = uint4{sel(v1.x, v1.z), sel(v1.y, v1.w), sel(v1.z, v1.x), sel(v1.w, v1.y)};
      gstore16_s<0>(Ob + hob, vo, v0);
      gstore16_s<1024>(Ob + hob, vo, v1);
      vmn += 2;
    }
  };
  // scalar counters: step g is row s of unit il, its tile at output byte tob; its refill
  // position g + 3 + LEAD is row sp - 1 of unit vp (the ilp-th)
  const unsigned ustride = (unsigned)G * HB * CT_TILE;
  int s = 0;
  unsigned tob = (unsigned)blockIdx.x * HB * CT_TILE, ub = tob;
  int ilp = (3 + LEAD) / SPI, sp = 3 + LEAD - ilp * SPI, vp = (int)blockIdx.x + ilp * G;
  // step g with g & 7 == I: ring slots and tile buffers are compile-time
  auto step = [&](auto ic) __attribute__((always_inline)) {
    constexpr int I = decltype(ic)::value;
    store_held(((I + 1) & 1) * CT_TILE);
    held = false;
    mk[LEAD] = stage_at((I + 3 + LEAD) & 7, ilp, vp, sp) ? ++vmn : -1;
    if (s < HB) {
      f32x4 acc[4] = {bias, bias, bias, bias};
      int u0[4] = {0, 8, 20, 32};
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const unsigned char* src = ring + ((I + 1 + dy) & 7) * C::ROWB;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          // K half 1 (groups kg + 4) sits at the half-0 offset ^ 64 bytes (swizzle bit 2)
          const uint4 b0 = *reinterpret_cast<const uint4*>(src + xo[dx + 1]);
          const uint4 b1 = *reinterpret_cast<const uint4*>(src + (xo[dx + 1] ^ 64));
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) acc[ph] = mfma16x16x32<T>(wf[u0[ph]], b0, acc[ph]);
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (ttap(ph, dy, dx)) {
              acc[ph] = mfma16x16x32<T>(wf[u0[ph] + 1], b1, acc[ph]);
              u0[ph] += 2;
            }
        }
      }
#pragma unroll
      for (int ph = 0; ph < 4; ++ph)
        *reinterpret_cast<uint2*>(tw + (I & 1) * CT_TILE + 4096 * (ph >> 1) + 128 * (ph & 1)) =
            relu_pack4<T>(acc[ph]);
      hob = tob;
      held = true;
    }
    // position g + 3 has landed (waves 0 and 1; steady state: 3 steps of 2 stores + 1 DMA
    // younger than it); the barrier also publishes the tile
    if (mk[0] >= 0) wait_vmcnt_ss<9>(vmn - mk[0]);
    lds_barrier();
#pragma unroll
    for (int i = 0; i < LEAD; ++i) mk[i] = mk[i + 1];
    tob += CT_TILE;
    if (++s == SPI) { s = 0; ub += ustride; tob = ub; }
    if (++sp == SPI) { sp = 0; ++ilp; vp += G; }
  };
  for (int g = 0; g < S; g += 8) {
    step(std::integral_constant<int, 0>{});
    if (g + 1 >= S) break;
    step(std::integral_constant<int, 1>{});
    if (g + 2 >= S) break;
    step(std::integral_constant<int, 2>{});
    if (g + 3 >= S) break;
    step(std::integral_constant<int, 3>{});
    if (g + 4 >= S) break;
    step(std::integral_constant<int, 4>{});
    if (g + 5 >= S) break;
    step(std::integral_constant<int, 5>{});
    if (g + 6 >= S) break;
    step(std::integral_constant<int, 6>{});
    if (g + 7 >= S) break;
    step(std::integral_constant<int, 7>{});
  }
  store_held(((S - 1) & 1) * CT_TILE);
}

// convt_rows_pg_kernel (variant CONVT_PG; measured SLOWER than convt_rows_pw_store8_kernel, 0.148 vs
// 0.130 ms per 2048 shots, profiles/r05_convt1_pg_ab.txt: kept for the record of the trial):
// convT1 with the four output phases split over two waves per 16-channel
// block (8 waves, one workgroup per CU): wave group A runs phases (0,0) and (1,1) (4 + 9 taps),
// group B phases (0,1) and (1,0) (6 + 6), so a wave holds 26 or 24 tap fragments (~100 VGPRs)
// instead of 50 and has the registers to read all of a step's B fragments (18 / 16) before its
// MFMAs: convt_rows_pw_store8_kernel read them in pairs right before use, exposing an LDS round
// trip per neighbourhood offset (PMC: MFMA busy 0.35). Each wave keeps its own input ring
// (LDS-DMA, no barrier in the step loop), as convt_rows_pw_store8_kernel.
template <typename T, int LEAD>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2)))
void convt_rows_pg_kernel(CRArgs a) {
  static_assert(LEAD >= 1 && LEAD <= 4, "8-row ring: positions g .. g + 3 + LEAD live");
  using C = TC<64, 16>;
  constexpr int CO = 64, W = 16;
  constexpr int WR = C::RING * C::ROWB;  // bytes per wave ring
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_pg[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int nb = wv & 3;
  unsigned char* const ring = lds_pg + wv * WR;
  const int H = a.H, SPI = H + 1;
  const int G = gridDim.x;
  const int nimg = ((int)a.N - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  for (int e = lane; e < WR / 16; e += 64) reinterpret_cast<uint4*>(ring)[e] = uint4{0u, 0u, 0u, 0u};
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // zero fill before the DMAs (other path)
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};
  int xo[3];  // byte offset of pixel m + dx (stored + 1), group kg, in a ring row
#pragma unroll
  for (int dx = -1; dx <= 1; ++dx) {
    const int ps = m + dx + 1;
    xo[dx + 1] = ps * 128 + 16 * (kg ^ (ps & 7));
  }
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  int dsrc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 64 * h + lane;
    const int ps = 1 + c / 8, gs = c & 7;
    dsrc[h] = (ps - 1) * 64 + 8 * (gs ^ (ps & 7));
  }
  auto stage_at = [&](int p, int il, int r) -> int {
    unsigned char* dst = ring + (p & 7) * C::ROWB + 128;
    if (il < nimg && r >= 0) {
      const long long n = (long long)blockIdx.x + (long long)il * G;
      const T* src = X + ((n * H + r) * W) * 64;
      lds_dma16_s(src, 2u * dsrc[0], dst);
      lds_dma16_s(src, 2u * dsrc[1], dst + 1024);
      return 2;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    *reinterpret_cast<uint4*>(dst + 1024 + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return 0;
  };
  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  constexpr int OW = 2 * W;

  // the wave group's program: phases PA, PB (compile time)
  auto run = [&](auto pa_c, auto pb_c) {
    constexpr int PA = decltype(pa_c)::value, PB = decltype(pb_c)::value;
    constexpr int PHS[2] = {PA, PB};
    // (dy, dx) offsets either phase uses, and the fragments: [phase slot][taps][K half]
    constexpr int NF = 2 * (((PA >> 1) + 2) * ((PA & 1) + 2) + ((PB >> 1) + 2) * ((PB & 1) + 2));
    uint4 wf[NF];
    {
      const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
      int u = 0;
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const int ph = PHS[q];
            if (!ttap(ph, dy, dx)) continue;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh)
              wf[u++] = *reinterpret_cast<const uint4*>(
                  Wg + (((16 * nb + m) * 5 + tky(ph >> 1, dy)) * 5 + tky(ph & 1, dx)) * 64 +
                  32 * kh + 8 * kg);
          }
    }
    resident_loads_landed();
#pragma unroll
    for (int p = 0; p < 3 + LEAD; ++p) {
      const int il = p / SPI;
      stage_at(p, il, p - il * SPI - 1);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    uint2 pk[2];
    long long po = 0;   // element offset of the held outputs' (2s, 2x) pixel
    bool held = false;  // (wave-uniform, as convt_rows_pw_kernel's)
    int vmn = 0;        // this wave's vector-memory ops issued in the loop
    int mk[LEAD + 1];   // vmn right after the DMAs of position g + 3 + i (-1: none in flight)
#pragma unroll
    for (int i = 0; i <= LEAD; ++i) mk[i] = -1;
    auto store_held = [&]() {
      if (held) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
          gstore8(O + po + ((PHS[q] >> 1) * OW + (PHS[q] & 1)) * CO, pk[q]);
        vmn += 2;
      }
    };
    int il = 0, s = 0;
    int ilp = (3 + LEAD) / SPI, sp = 3 + LEAD - ilp * SPI;
    for (int g = 0; g < S; ++g) {
      store_held();
      held = false;
      const int nd = stage_at(g + 3 + LEAD, ilp, sp - 1);
      vmn += nd;
      mk[LEAD] = nd ? vmn : -1;
      if (s < H) {
        uint4 bq[9][2];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const unsigned char* src = ring + ((g + 1 + dy) & 7) * C::ROWB;
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            if (!ttap(PA, dy, dx) && !ttap(PB, dy, dx)) continue;
            bq[3 * (dy + 1) + dx + 1][0] = *reinterpret_cast<const uint4*>(src + xo[dx + 1]);
            bq[3 * (dy + 1) + dx + 1][1] = *reinterpret_cast<const uint4*>(src + (xo[dx + 1] ^ 64));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[2] = {bias, bias};
        int u0[2] = {0, NF / 2 - 0};
        u0[1] = 2 * ((PA >> 1) + 2) * ((PA & 1) + 2);
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
            for (int q = 0; q < 2; ++q)
              if (ttap(PHS[q], dy, dx)) {
                acc[q] = mfma16x16x32<T>(wf[u0[q]], bq[3 * (dy + 1) + dx + 1][0], acc[q]);
                acc[q] = mfma16x16x32<T>(wf[u0[q] + 1], bq[3 * (dy + 1) + dx + 1][1], acc[q]);
                u0[q] += 2;
              }
#pragma unroll
        for (int q = 0; q < 2; ++q) pk[q] = relu_pack4<T>(acc[q]);
        const long long n = (long long)blockIdx.x + (long long)il * G;
        po = ((n * 2 * H + 2 * s) * OW + 2 * m) * CO + 16 * nb + 4 * kg;
        held = true;
      }
      if (mk[0] >= 0) wait_vmcnt(vmn - mk[0]);
      asm volatile("" ::: "memory");
#pragma unroll
      for (int i = 0; i < LEAD; ++i) mk[i] = mk[i + 1];
      if (++s == SPI) { s = 0; ++il; }
      if (++sp == SPI) { sp = 0; ++ilp; }
    }
    store_held();
  };
  if (wv < 4)
    run(std::integral_constant<int, 0>{}, std::integral_constant<int, 3>{});
  else
    run(std::integral_constant<int, 1>{}, std::integral_constant<int, 2>{});
}

template <typename T>
hipError_t launch_convt_rows_pg(const CRArgs& a, hipStream_t st) {
  using C = TC<64, 16>;
  constexpr int LDS = 8 * C::RING * C::ROWB;
  static LdsOptIn lds_site;
  const hipError_t e =
      allow_lds(lds_site, {reinterpret_cast<const void*>(&convt_rows_pg_kernel<T, 3>)}, LDS);
  if (e != hipSuccess) return e;
  const long long grid = std::min<long long>(a.N, (long long)device_cus());
  SPECENH_LAUNCH((convt_rows_pg_kernel<T, 3>), dim3((unsigned)grid), dim3(512), LDS, st, a);
  return hipGetLastError();
}

// log2 of the row bands per image for the convT row sweeps: whole images while the batch
// fills the resident workgroup slots; a small batch (C4's 128 images: 128 workgroups for 512
// slots) is cut into up to 8 bands of >= 4 rows (two bubble steps and two halo rows each)
int convt_row_bands_lg(int N, int H, long long slots) {
  const int forced = variant(V_ROWS_BANDS);
  int lg = 0;
  while (lg < 3 && (H % (2 << lg)) == 0 && (H >> (lg + 1)) >= 4 &&
         (forced >= 0 ? lg < forced : ((long long)N << (lg + 1)) <= slots))
    ++lg;
  return lg;
}

// convT1's per-workgroup-of-4-waves kernels: staged whole-line stores (default) or the per-wave
// rings with 8-byte stores (STORE8)
template <typename T, bool STORE8>
hipError_t launch_convt_rows_pw(const CRArgs& a0, hipStream_t st) {
  using C = TC<64, 16>;
  constexpr int LDS = STORE8 ? 4 * C::RING * C::ROWB : C::LDS + 2 * CT_TILE;
  const void* k = STORE8 ? reinterpret_cast<const void*>(&convt_rows_pw_store8_kernel<T, 3>)
                         : reinterpret_cast<const void*>(&convt_rows_pw_kernel<T, 3>);
  static LdsOptIn lds_site;
  static ResidentSlots site;
  long long slots = 0;
  hipError_t e = allow_lds(lds_site, {k}, LDS);
  if (e == hipSuccess) e = resident_slots(site, k, 256, LDS, &slots);
  if (e != hipSuccess) return e;
  CRArgs a = a0;
  a.lgb = convt_row_bands_lg(a.N, a.H, slots);
  const long long grid = std::min<long long>((long long)a.N << a.lgb, slots);
  if constexpr (STORE8)
    SPECENH_LAUNCH((convt_rows_pw_store8_kernel<T, 3>), dim3((unsigned)grid), dim3(256), LDS, st, a);
  else
    SPECENH_LAUNCH((convt_rows_pw_kernel<T, 3>), dim3((unsigned)grid), dim3(256), LDS, st, a);
  return hipGetLastError();
}

template <typename T, int CO, int W, int LEAD>
hipError_t launch_convt_rows_lead(const CRArgs& a0, hipStream_t st) {
  using C = TC<CO, W>;
  const void* k = reinterpret_cast<const void*>(&convt_rows_kernel<T, CO, W, LEAD>);
  static ResidentSlots site;
  long long slots = 0;
  const hipError_t e = resident_slots(site, k, C::THREADS, C::LDS, &slots);
  if (e != hipSuccess) return e;
  CRArgs a = a0;
  a.lgb = convt_row_bands_lg(a.N, a.H, slots);
  const long long grid = std::min<long long>((long long)a.N << a.lgb, slots);
  SPECENH_LAUNCH((convt_rows_kernel<T, CO, W, LEAD>), dim3((unsigned)grid), dim3(C::THREADS),
                 C::LDS, st, a);
  return hipGetLastError();
}

template <typename T, int CO, int W>
hipError_t launch_convt_rows(const CRArgs& a, hipStream_t st) {
  return variant(V_ROWS_SHORT_LEAD) ? launch_convt_rows_lead<T, CO, W, 1>(a, st)
                               : launch_convt_rows_lead<T, CO, W, 3>(a, st);
}

// ============================================================================ convT rows, 32 in
// convt_rows32_kernel: Conv2DTranspose(CO, K, strides=2, relu, same) on 32-channel inputs as a
// row sweep, K = 3 / 5 / 7 — the decoders' first Conv2DTranspose of the reference's scan models
// (VAE/hyperparam_scan.py:160 and manual_scan.py:197: 32 -> 32 at 64 x 32 -> 128 x 64 for their
// 256 x 128 inputs), which conv_patch_kernel ran at 0.06-0.19 of the MFMA peak. The schedule of
// convt_rows_kernel with the kernel size generalised: output phase (py, px) of position (s, x)
// reads input row s + dy with tap ky = 2 dy + PT - py (PT = K - 1 - (K - 2) / 2, the dilated
// conv's pad), so each neighbourhood offset's ONE B fragment (32 channels: one K step) feeds
// every phase that has the tap, exactly the K^2 useful taps per (row, 16 positions, 16 output
// channels). Positions: row r of the workgroup's image il at il SPI + r - DY0, SPI = H +
// max(DY1, -DY0) (zero rows between images), so step g reads positions g .. g + NDY - 1.
// Input pixels are 64 B with their 16-byte groups swizzled by (p >> 1) & 3 (conflict-free
// fragment reads at any offset, tools/lds_banks.py).
template <int CO, int W, int K>
struct TC32 {
  static constexpr int CI = 32;
  static constexpr int NWIN = W / 16, NNB = CO / 16;
  static constexpr int WAVES = NWIN * NNB;
  static constexpr int THREADS = 64 * WAVES;
  static constexpr int PT = K - 1 - (K - 2) / 2;
  static constexpr int ky_of(int py, int dy) { return 2 * dy + PT - py; }
  static constexpr bool tap(int ph, int dy, int dx) {
    return ky_of(ph >> 1, dy) >= 0 && ky_of(ph >> 1, dy) < K && ky_of(ph & 1, dx) >= 0 &&
           ky_of(ph & 1, dx) < K;
  }
  static constexpr bool any_tap(int dy, int dx) {
    return tap(0, dy, dx) || tap(1, dy, dx) || tap(2, dy, dx) || tap(3, dy, dx);
  }
  static constexpr int DY0 = -(PT / 2), DY1 = (K - PT) / 2;  // neighbourhood rows (and columns)
  static constexpr int NDY = DY1 - DY0 + 1;
  static constexpr int GAP = DY1 > -DY0 ? DY1 : -DY0;       // zero rows between images
  static constexpr int tap_index(int ph, int dy, int dx) {  // phase-major, (dy, dx) row-major
    int u = 0;
    for (int p = 0; p < 4; ++p)
      for (int a = DY0; a <= DY1; ++a)
        for (int b = DY0; b <= DY1; ++b) {
          if (p == ph && a == dy && b == dx) return u;
          if (tap(p, a, b)) ++u;
        }
    return -1;
  }
  static constexpr int ROWB = (W + NDY - 1) * CI * 2;  // pixels x = DY0 .. W - 1 + DY1
  static constexpr int RING = 8;
  static constexpr int LDS = RING * ROWB;
  static constexpr int DMA_WAVES = W * CI * 2 / 1024;  // one 1-KB DMA per wave and row
  static_assert(WAVES == 4 && DMA_WAVES <= WAVES && (W * CI * 2) % 1024 == 0, "shape");
  static_assert(tap(3, DY0, DY0) || tap(0, DY0, DY0) || any_tap(DY0, 0), "neighbourhood");
};

__device__ __forceinline__ int x32off(int ps, int g) { return ps * 64 + 16 * (g ^ ((ps >> 1) & 3)); }

template <typename T, int CO, int W, int K, int LEAD>
__global__ __launch_bounds__((TC32<CO, W, K>::THREADS)) __attribute__((amdgpu_waves_per_eu(2)))
void convt_rows32_kernel(CRArgs a) {
  using C = TC32<CO, W, K>;
  constexpr int DY0 = C::DY0, DY1 = C::DY1, NDY = C::NDY;
  static_assert(LEAD >= 1 && NDY + LEAD + 1 <= C::RING, "ring: positions g .. g + NDY + LEAD live");
  extern __shared__ __attribute__((aligned(16))) unsigned char ring[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int wx = wv % C::NWIN, nb = wv / C::NWIN;
  const int H = a.H, SPI = H + C::GAP;
  const int G = gridDim.x;
  const int nimg = ((int)a.N - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  {
    uint4* z = reinterpret_cast<uint4*>(ring);
    for (int e = tid; e < C::LDS / 16; e += C::THREADS) z[e] = uint4{0u, 0u, 0u, 0u};
  }
  uint4 wf[K * K];  // tap fragments, phase-major
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w);
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
      for (int dy = DY0; dy <= DY1; ++dy)
#pragma unroll
        for (int dx = DY0; dx <= DY1; ++dx)
          if (C::tap(ph, dy, dx))
            wf[C::tap_index(ph, dy, dx)] = *reinterpret_cast<const uint4*>(
                Wg + (((16 * nb + m) * K + C::ky_of(ph >> 1, dy)) * K + C::ky_of(ph & 1, dx)) * 32 +
                8 * kg);
  }
  const f32x4 bias = f32x4{a.b[16 * nb + 4 * kg], a.b[16 * nb + 4 * kg + 1],
                           a.b[16 * nb + 4 * kg + 2], a.b[16 * nb + 4 * kg + 3]};
  resident_loads_landed();
  int xo[NDY];  // byte offset of pixel 16 wx + m + dx (stored x - DY0), group kg, in a ring row
#pragma unroll
  for (int dx = DY0; dx <= DY1; ++dx) xo[dx - DY0] = x32off(16 * wx + m + dx - DY0, kg);
  // ring refill: wave w < DMA_WAVES moves chunks 64 w .. 64 w + 63 (pixels 16 w .. 16 w + 15)
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  const bool dma_wave = wv < C::DMA_WAVES;
  int dsrc = 0;
  if (dma_wave) {
    const int c = 64 * wv + lane;
    const int x = c / 4, gs = c & 3, ps = x - DY0;
    dsrc = x * 32 + 8 * (gs ^ ((ps >> 1) & 3));
  }
  // stream position p = il SPI + r - DY0 -> ring slot p & 7 (a zero row unless 0 <= r < H)
  auto stage_at = [&](int p, int il, int r) -> bool {
    if (!dma_wave) return false;
    unsigned char* dst = ring + (p & 7) * C::ROWB + (-DY0) * 64 + 1024 * wv;
    if (il < nimg && r >= 0 && r < H) {
      const long long n = (long long)blockIdx.x + (long long)il * G;
      lds_dma16_s(X + ((n * H + r) * W) * 32, 2u * dsrc, dst);
      return true;
    }
    *reinterpret_cast<uint4*>(dst + 16 * lane) = uint4{0u, 0u, 0u, 0u};
    return false;
  };
  auto stage = [&](int p) -> bool {  // (prologue)
    const int il = p / SPI;
    return stage_at(p, il, p - il * SPI + DY0);
  };
  __syncthreads();  // ring zeroed
#pragma unroll
  for (int p = 0; p < NDY + LEAD; ++p) stage(p);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();

  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int OW = 2 * W;
  uint2 pk[4];
  long long po = 0;   // element offset of the held outputs' (2s, 2x) pixel
  bool held = false;  // (wave-uniform, as convt_rows_pw_kernel's)
  int vmn = 0;        // this wave's vector-memory ops issued in the loop
  int mk[LEAD + 1];   // vmn right after the DMA of position g + NDY + i (-1: none in flight)
#pragma unroll
  for (int i = 0; i <= LEAD; ++i) mk[i] = -1;
  auto store_held = [&]() {
    if (held) {
#pragma unroll
      for (int ph = 0; ph < 4; ++ph)
        gstore8(O + po + ((ph >> 1) * OW + (ph & 1)) * CO, pk[ph]);
      vmn += 4;
    }
  };
  // scalar counters (image, step in image) of step g and of its refill position g + NDY + LEAD
  int il = 0, s = 0;
  int ilp = (NDY + LEAD) / SPI, sp = NDY + LEAD - ilp * SPI;
  for (int g = 0; g < S; ++g) {
    store_held();
    held = false;
    mk[LEAD] = stage_at(g + NDY + LEAD, ilp, sp + DY0) ? ++vmn : -1;
    if (s < H) {
      f32x4 acc[4] = {bias, bias, bias, bias};
#pragma unroll
      for (int dy = DY0; dy <= DY1; ++dy) {
        const unsigned char* src = ring + ((g + dy - DY0) & 7) * C::ROWB;
#pragma unroll
        for (int dx = DY0; dx <= DY1; ++dx) {
          if (!C::any_tap(dy, dx)) continue;
          const uint4 b = *reinterpret_cast<const uint4*>(src + xo[dx - DY0]);
#pragma unroll
          for (int ph = 0; ph < 4; ++ph)
            if (C::tap(ph, dy, dx)) acc[ph] = mfma16x16x32<T>(wf[C::tap_index(ph, dy, dx)], b, acc[ph]);
        }
      }
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) pk[ph] = relu_pack4<T>(acc[ph]);
      const long long n = (long long)blockIdx.x + (long long)il * G;
      po = ((n * 2 * H + 2 * s) * OW + 2 * (16 * wx + m)) * CO + 16 * nb + 4 * kg;
      held = true;
    }
    if (mk[0] >= 0) wait_vmcnt_ss<15>(vmn - mk[0]);  // position g + NDY has landed
    lds_barrier();
#pragma unroll
    for (int i = 0; i < LEAD; ++i) mk[i] = mk[i + 1];
    if (++s == SPI) { s = 0; ++il; }
    if (++sp == SPI) { sp = 0; ++ilp; }
  }
  store_held();
}

template <typename T, int CO, int W, int K>
hipError_t launch_convt_rows32(const CRArgs& a, hipStream_t st) {
  using C = TC32<CO, W, K>;
  constexpr int LEAD = 8 - C::NDY - 1 < 3 ? 8 - C::NDY - 1 : 3;
  const void* k = reinterpret_cast<const void*>(&convt_rows32_kernel<T, CO, W, K, LEAD>);
  static ResidentSlots site;
  long long slots = 0;
  const hipError_t e = resident_slots(site, k, C::THREADS, C::LDS, &slots);
  if (e != hipSuccess) return e;
  const long long grid = std::min<long long>(a.N, slots);
  SPECENH_LAUNCH((convt_rows32_kernel<T, CO, W, K, LEAD>), dim3((unsigned)grid),
                 dim3(C::THREADS), C::LDS, st, a);
  return hipGetLastError();
}

// ============================================================================ C = 1 rows
// The first Conv2D(16, 5, relu, same) + MaxPooling2D(2) (VAE/manual_scan_3layers.py:187-188)
// on W = 128 one-channel images, as a row sweep. Lane m of wave w owns pooled pixel
// p = 16 w + m, that is output columns x = 2p + cb (cb = 0, 1), which read input columns
// 2p - 2 .. 2p + 2 and 2p - 1 .. 2p + 3: together a six-column window from the even column
// 2p - 2, three whole words of the staged row. The column parity is in the weights, not the
// data: 5 kernel rows x 6 window columns = 30 of the 32 K slots of ONE 16x16x32 MFMA, and both
// parities of an output row share one B fragment. K-slot map (lane group g, slot j = 0 .. 7, A
// and B alike; c1_afrag / c1_bword below, restated in tests/test_conv1_pack_mapping.py):
//    j < 6           kernel row g, window column j
//    j = 6, 7, g < 3 kernel row 4, window column 2g + j - 6
//    j = 6, 7, g = 3 weight zero; the lane reads a word that is always zero
// A[cb] holds w[ch][ky][kx] at window column kx + cb (zero at the column the parity does not
// reach), so output row y = 2p' + dy is acc[dy][cb] = A[cb] x B(y) + bias: 4 MFMAs per wave and
// step (pooled row p'), all 25 taps each, the 2 x 2 pool in the lane's own four accumulators,
// no cross-lane exchange, 8-byte stores of whole 512-byte pixel runs per wave. conv_c1_mfma
// tiles 32 x 32 with a halo and re-read the input 3.3x (PMC); here every row is read once.
//  * a staged row holds elements x = -8 .. W + 5 (zero outside the image) once, as 32-bit words
//    as loaded: x = 0 is word 4, the window of pixel p words p + 3 .. p + 5. The B fragment of
//    output row y (rows y - 2 .. y + 2 at positions pos .. pos + 4) is four ds_read_b32 per
//    lane (m, g): words p + 3, p + 4, p + 5 of row pos + g and word p + 3 + g of row pos + 4
//    (g = 3: the zero word). Rows are C1ROW = 80 = 16 (mod 32) words apart: the two rows of a
//    half-wave read disjoint banks, row pos + 4's overlapping reads are identical words
//    (broadcast), and the zero word (word 72 of row pos + 3 or pos + 4, a pad no DMA writes;
//    the row by the wave's parity) sits in the 16 banks lane group 2 leaves free: every read
//    is conflict-free at every ring position (tools/lds_banks.py);
//  * the rows are one stream per workgroup: position il (H + 4) + r + 2 holds row r of the
//    workgroup's image il (two zero rows above and below each image), step g = il (H/2 + 2)
//    + p reads positions 2g .. 2g + 5 (p >= H/2: bubbles); LDS-DMA 5 steps ahead into a
//    16-row ring (waited for two steps later).
// Finite inputs are the contract. A zero weight multiplies window column 5 (cb = 0) or 0
// (cb = 1), and row pos + 4's columns outside the parity's five: an Inf or NaN pixel there
// reaches the other parity's accumulator of the same pool window (0 x Inf = NaN), where a
// per-tap sum would not see it.
constexpr int C1W = 128;   // image width
constexpr int C1ROW = 80;  // words per staged row: elements x = -8 .. W + 5 in words 0 .. 70
constexpr int C1ZW = 72;   // a word of the row's tail pad (words 71 .. 79: never written)
constexpr int C1RING = 16;
constexpr int C1LDS = C1RING * C1ROW * 4;

// A fragment of column parity cb for lane (channel m, lane group g); Wg: [16][5][5]
template <typename T>
__device__ __forceinline__ uint4 c1_afrag(const T* __restrict__ Wg, int m, int g, int cb) {
  uint32_t q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * i + h;
      const int ky = j < 6 ? g : 4, c = (j < 6 ? j : 2 * g + j - 6) - cb;
      v[h] = (j < 6 || g < 3) && c >= 0 && c <= 4 ? (float)Wg[(m * 5 + ky) * 5 + c] : 0.f;
    }
    q[i] = pack2_cvt<T>(v[0], v[1]);
  }
  return uint4{q[0], q[1], q[2], q[3]};
}
// The fourth word of lane (pixel p of pixel block w, lane group g)'s B fragment is word
// c1_k4word of the row c1_k4row positions below the fragment's first: kernel row 4's columns
// 2g, 2g + 1, or the zero word
__device__ __forceinline__ int c1_k4row(int w, int g) { return g < 3 ? 4 : 3 + (w & 1); }
__device__ __forceinline__ int c1_k4word(int p, int g) { return g < 3 ? p + 3 + g : C1ZW; }
// (volatile: four separate ds_read_b32; paired into ds_read2_b32 they cost more LDS cycles)
typedef __attribute__((address_space(3))) const volatile uint32_t c1_lds_u32;
__device__ __forceinline__ uint4 c1_bfrag(const uint32_t* run, const uint32_t* k4) {
  c1_lds_u32* r = (c1_lds_u32*)run;
  c1_lds_u32* r4 = (c1_lds_u32*)k4;
  const uint32_t a = r[0], b = r[1], c = r[2], d = r4[0];
  return uint4{a, b, c, d};
}

template <typename T>
__global__ __launch_bounds__(256) void conv1_rows_pool_kernel(CRArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ring_raw[];
  uint32_t* const ring = reinterpret_cast<uint32_t*>(ring_raw);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int H = a.H, SPI = H / 2 + 2, PPI = H + 4;
  const int G = gridDim.x;
  const int nimg = ((int)a.N - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI;

  for (int e = tid; e < C1RING * C1ROW; e += 256) ring[e] = 0u;
  // A operands: lane (m, kg) = channel m, one fragment per column parity
  const uint4 w0 = c1_afrag<T>(reinterpret_cast<const T*>(a.w), m, kg, 0);
  const uint4 w1 = c1_afrag<T>(reinterpret_cast<const T*>(a.w), m, kg, 1);
  const f32x4 bias = f32x4{a.b[4 * kg], a.b[4 * kg + 1], a.b[4 * kg + 2], a.b[4 * kg + 3]};

  // ring refill (wave 0): positions pp, pp + 1 by LDS-DMA, 16 B (8 elements) per lane from
  // lanes 0-15, into words 4 .. 67 (x = 0 .. W - 1); returns the DMAs issued
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  auto stage = [&](int pp) -> int {
    if (wv != 0) return 0;
    int nd = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int pos = pp + j;
      const int il = pos / PPI, r = pos - il * PPI - 2;
      uint32_t* dst = ring + (pos & (C1RING - 1)) * C1ROW + 4;  // x = 0 is word 4
      if (il < nimg && r >= 0 && r < H) {
        const long long n = (long long)blockIdx.x + (long long)il * G;
        if (lane < 16) lds_dma16(X + (n * H + r) * C1W + 8 * lane, dst);
        ++nd;
      } else if (lane < 16) {
        *reinterpret_cast<uint4*>(dst + 4 * lane) = uint4{0u, 0u, 0u, 0u};
      }
    }
    return nd;
  };
  __syncthreads();  // ring zeroed
  for (int pp = 0; pp < 10; pp += 2) stage(pp);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();

  // B fragment of the output row whose five input rows are at positions pos .. pos + 4
  const int wbase = 16 * wv + m + 3;
  const int k4r = c1_k4row(wv, kg), k4w = c1_k4word(16 * wv + m, kg);
  auto bfrag = [&](int pos) -> uint4 {
    return c1_bfrag(ring + ((pos + kg) & (C1RING - 1)) * C1ROW + wbase,
                    ring + ((pos + k4r) & (C1RING - 1)) * C1ROW + k4w);
  };
  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int PW = C1W / 2, PH = H / 2;
  for (int g = 0; g < S; ++g) {
    // positions 2g + 10, 2g + 11 into the ring (their slots held 2g - 6, 2g - 5: done)
    const int nd = stage(2 * g + 10);
    const int il = g / SPI, p = g - il * SPI;
    if (p < PH) {
      const int pb = 2 * g;  // position of input row 2p - 2
      // output rows y = 2p + dy: both fragments before the first MFMA
      const uint4 b0 = bfrag(pb), b1 = bfrag(pb + 1);
      f32x4 acc[2][2];
      acc[0][0] = mfma16x16x32<T>(w0, b0, bias);
      acc[0][1] = mfma16x16x32<T>(w1, b0, bias);
      acc[1][0] = mfma16x16x32<T>(w0, b1, bias);
      acc[1][1] = mfma16x16x32<T>(w1, b1, bias);
      float v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = fmaxf(fmaxf(fmaxf(acc[0][0][i], acc[0][1][i]), fmaxf(acc[1][0][i], acc[1][1][i])),
                     0.f);
      const long long n = (long long)blockIdx.x + (long long)il * G;
      *reinterpret_cast<uint2*>(O + ((n * PH + p) * PW + 16 * wv + m) * 16 + 4 * kg) =
          uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])};
    }
    // wave 0: the DMAs of step g - 1 (positions 2g + 8, 2g + 9, first read at step g + 2) must
    // land before the barrier; this step's DMAs and its store are the youngest vector-memory
    // ops, so wait for all but those. The other waves issue only stores: no wait.
    if (wv == 0) {
      const int younger = nd + (p < PH ? 1 : 0);
      if (younger == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (younger == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else if (younger == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    }
    lds_barrier();
  }
}

template <typename T>
hipError_t launch_conv1_rows(const CRArgs& a, hipStream_t st) {
  const void* k = reinterpret_cast<const void*>(&conv1_rows_pool_kernel<T>);
  static ResidentSlots site;
  long long slots = 0;
  const hipError_t e = resident_slots(site, k, 256, C1LDS, &slots);
  if (e != hipSuccess) return e;
  const long long grid = std::min<long long>(a.N, slots);
  SPECENH_LAUNCH(conv1_rows_pool_kernel<T>, dim3((unsigned)grid), dim3(256), C1LDS, st, a);
  return hipGetLastError();
}

// ============================================================================ encoder 1+2
// The encoder's first two layers in one launch (VAE/manual_scan_3layers.py:187-191):
// Conv2D(16, 5, relu) + MaxPooling2D(2) on 128 x 128 one-channel images, then Conv2D(32, 5,
// relu) + MaxPooling2D(2). The 64 x 64 x 16 map between them (128 KB per image, written and
// read once each by the two-launch path) is produced in conv2's LDS ring and never reaches
// HBM. The conv2 part is conv_rows_pool_kernel<T, 16, 32, 64> step for step; instead of an
// LDS-DMA of its input rows, step s computes the two conv2 input rows of step s + 2 with
// the conv1 row sweep (conv1_rows_pool_kernel: waves 0-3 the first row, 4-7 the second,
// 16 pooled pixels each: 4 MFMAs per wave on two gathered B fragments, the same A and B
// operands as conv1_rows_pool_kernel's for every accumulator, so the two paths agree bit for
// bit) from a 32-row stream of the images' rows (4 per step: H + 4 = 4 (H/4 + 1) positions per
// image), LDS-DMA 8 steps ahead. As there, finite inputs are the contract: a zero weight
// multiplies the window's column of the other parity, so an Inf or NaN pixel reaches both
// column parities of its pool window.
struct E2Args {
  const void* x;    // [N][H][128] (C = 1)
  const void* w1;   // conv1 GEMM weights [16][5][5]
  const float* b1;  // [16]
  const void* w2;   // conv2 GEMM weights [32][5][5][16]
  const float* b2;  // [32]
  void* out;        // [N][H/4][32][32]
  int N, H;
};

// conv1 input ring rows (positions), each staged once as in conv1_rows_pool_kernel (C1ROW
// words; the zero word of a B fragment is a row's own tail pad, so the ring needs no zero row)
constexpr int E2R1 = 32;
#ifndef SPECENH_ENC2_STAGGER
#define SPECENH_ENC2_STAGGER 0
#endif

constexpr int E2LDS = RC<16, 32, 64>::LDS + E2R1 * C1ROW * 4 + 48 * 4;  // rings + biases
// Schedule 1's pooled-row tiles: a step's pooled row (32 pixels x 32 channels, 2 KB contiguous
// in the NHWC output), double-buffered behind the rings and the biases. Wave (wx, nb), lane
// (m, kg) writes the 8 bytes of channels 16 nb + 4 kg .. + 3 of pixel p = (16 wx + m) / 2 (8-byte
// chunk c8 = 4 nb + kg of the pixel's 64 bytes) at chunk c8 ^ 2 ((p >> 1) & 3): the eight
// pixels of a ds_write_b64 lane group then cover 32 distinct banks (a plain 64-byte pitch is
// 4-way), and 16-byte units move whole, so the read-back needs no half swap. Store wave k, lane
// l reads the 16 bytes of output byte 1024 k + 16 l (pixel 16 k + l / 4, unit l & 3): the four
// lanes of a pixel cover its 64 bytes, conflict-free under the ds_read_b128 lane groups.
// (restated and checked in tests/test_enc2_stage_mapping.py)
constexpr int E2TILE = 32 * 32 * 2;
constexpr int E2LDS1 = E2LDS + 2 * E2TILE;
__host__ __device__ constexpr int e2_tile_write(int p, int c8) {
  return 64 * p + 8 * (c8 ^ (2 * ((p >> 1) & 3)));
}
__host__ __device__ constexpr int e2_tile_read(int k, int l) {
  const int p = 16 * k + (l >> 2);
  return 64 * p + 16 * ((l & 3) ^ ((p >> 1) & 3));
}

// max of two packed pairs of T as signed 16-bit integers: a non-negative T orders as its
// bits do and every negative one sorts below +0, so max(max(x, y), 0) = round(relu(max)) of the
// fp32 values x and y were rounded from (rounding is monotone), with -0 -> +0 as fmaxf(., 0).
// That holds for finite values and infinities. A NaN differs: fmaxf drops it, here one with a
// clear sign bit sorts above every number and reaches the output.
__device__ __forceinline__ uint32_t max_s16x2(uint32_t x, uint32_t y) {
  typedef short s2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(s2, x),
                                                                __builtin_bit_cast(s2, y)));
}

// WPE: waves per SIMD the register budget is cut for (4: two workgroups per CU, 128 VGPRs;
// 2: one workgroup, 256 VGPRs)
//
// SCHED: the step's schedule (variant ENC2_SCHED; as conv_rows_pool_kernel's, every wave runs
// the same program and all eight meet at one barrier per step, so the time of a step is the
// time one wave takes to get through it).
//  0 (the step until round 8, kept as the A/B and bitwise partner, and the WPE = 2 build's):
//    every step opens with the pool of pair s - 2 and its 8-byte store, whose address, like
//    the DMA's source row, is rebuilt from (image, row) with 64-bit multiplies; the counters
//    and image-boundary tests follow the barrier; conv1 and conv2 are separate blocks.
//  1 (WPE = 4 only): the store base and the DMA source row are 64-bit scalar pointers
//    advanced by adds (one per step, the jump to the workgroup's next image at a boundary); the
//    counters and the wave-uniform tests of step s + 1 are folded into one flag word under
//    step s's MFMAs; the pooled row goes to an LDS tile (e2_tile_write) and leaves one step
//    later as two 1 KB whole-line stores by waves 6 and 7 (two of the waves with no DMA), so
//    no wave's step opens with a store and the DMA waves' vmcnt ledger counts DMAs only;
//    conv2's pool and ReLU run on packed 16-bit pairs, in one block with the tile write, the
//    bookkeeping and conv1's fragment reads (both B fragments at the top of the block); the
//    bubble's and the image top's F fragments are zeroed by address select. The order pool,
//    conv1, conv2 is schedule 0's. Every accumulator keeps its order of MFMAs and every value
//    its roundings: for finite accumulators (and infinities) bitwise equal to 0; a NaN
//    accumulator, which schedule 0's fmaxf drops, can reach the output (max_s16x2).
//    (A hand-ordered block with fragments read further ahead did not fit 128 VGPRs: DESIGN.md
//    section 7.7.)
template <typename T, int WPE, int SCHED = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE)))
void enc2_rows_kernel(E2Args a) {
  static_assert(SCHED == 0 || (SCHED == 1 && WPE == 4), "schedule");
  using C = RC<16, 32, 64>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* const ring = lds;                                        // conv2 input rows
  uint32_t* const ring1 = reinterpret_cast<uint32_t*>(lds + C::LDS);     // image rows
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, kg = lane >> 4;
  const int wx = wv % C::NWIN, nb = wv / C::NWIN;
  const int x0 = 16 * wx;
  const int H1 = a.H, H = H1 / 2;           // conv1 / conv2 input heights
  const int SPI = H / 2 + 1, PPI = H1 + 4;  // conv2 steps and image-row positions per image
  const int G = gridDim.x;
  const int nimg = ((int)a.N - (int)blockIdx.x + G - 1) / G;
  const int S = nimg * SPI + 1;

  for (int e = tid; e < (C::LDS + E2R1 * C1ROW * 4) / 16; e += 512)
    reinterpret_cast<uint4*>(lds)[e] = uint4{0u, 0u, 0u, 0u};
  // both layers' biases in LDS (read where used: as resident f32x4s they cost the 8 VGPRs
  // that made the 4-waves-per-SIMD build spill)
  float* const btab = reinterpret_cast<float*>(lds + C::LDS + E2R1 * C1ROW * 4);
  if (tid < 16) btab[tid] = a.b1[tid];
  else if (tid < 48) btab[tid] = a.b2[tid - 16];
  auto bias2_ld = [&]() { return *reinterpret_cast<const f32x4*>(btab + 16 + 16 * nb + 4 * kg); };

  // ---- conv2: resident weight fragments (as conv_rows_pool_kernel, CIN = 16) ----
  uint4 wf[13];
  {
    const T* __restrict__ Wg = reinterpret_cast<const T*>(a.w2);
    const int co = 16 * nb + m, hi = kg >> 1, c8 = 8 * (kg & 1);
    auto tap = [&](int ky, int kx) {
      return *reinterpret_cast<const uint4*>(Wg + ((co * 5 + ky) * 5 + kx) * 16 + c8);
    };
#pragma unroll
    for (int ky = 0; ky < 5; ++ky) {
      wf[ky] = tap(ky, hi);
      wf[5 + ky] = tap(ky, 2 + hi);
    }
    wf[10] = tap(hi, 4);
    wf[11] = tap(2 + hi, 4);
    wf[12] = hi ? uint4{0u, 0u, 0u, 0u} : tap(4, 4);
  }

  const int boff = (x0 + m + (kg >> 1)) * 32 + 16 * (kg & 1);
  const int fo = (x0 + m + 4) * 32 + 16 * (kg & 1);
  const int foff = fo + (kg >> 1) * C::ROWB, foffw = fo - (kg >> 1) * 7 * C::ROWB;

  // ---- conv1: A fragments of column parity 0 / 1 (conv1_rows_pool_kernel's) ----
  const uint4 v0 = c1_afrag<T>(reinterpret_cast<const T*>(a.w1), m, kg, 0);
  const uint4 v1 = c1_afrag<T>(reinterpret_cast<const T*>(a.w1), m, kg, 1);
  resident_loads_landed();
  const int w1x = wv & 3, jr = wv >> 2;  // conv1 pixel block, conv2 input row of the pair
  // this lane's words of a B fragment at position pos: words p + 3 .. p + 5 of ring row
  // pos + kg and the fourth word, as byte offsets from ring row pos (two lane registers; the
  // wrap past the ring's end is an unsigned min: see bfrag)
  const uint32_t boA = (kg * C1ROW + 16 * w1x + m + 3) * 4;
  const uint32_t boK = (c1_k4row(w1x, kg) * C1ROW + c1_k4word(16 * w1x + m, kg)) * 4;

  // image-row stream: position pp = il (H1 + 4) + y + 2; waves 0-3 move positions pp + wv.
  // The loop keeps (image, row) of its positions and steps as scalar counters advanced per
  // step (a run-time division per use had cost ~25 SALU + a VALU reciprocal each).
  const T* __restrict__ X = reinterpret_cast<const T*>(a.x);
  auto stage1_at = [&](int pos, int il, int y) -> int {  // position pos = il PPI + y + 2
    uint32_t* dst = ring1 + (pos & (E2R1 - 1)) * C1ROW + 4;
    if (il < nimg && y >= 0 && y < H1) {
      const long long n = (long long)blockIdx.x + (long long)il * G;
      // wave-uniform row base + 16 B per lane (SGPR base, no 64-bit lane address to keep)
      if (lane < 16) lds_dma16_s(X + (n * H1 + y) * C1W, 16u * lane, dst);
      return 1;
    }
    // a zero formed at the store: as a loop-invariant uint4 it was hoisted and spilled
    int z = 0;
    asm volatile("" : "+v"(z));
    if (lane < 16) *reinterpret_cast<uint4*>(dst + 4 * lane) = uint4{(uint32_t)z, (uint32_t)z, (uint32_t)z, (uint32_t)z};
    return 0;
  };
  auto stage1 = [&](int pp) -> int {  // (prologue)
    if (wv >= 4) return 0;
    const int pos = pp + wv;
    const int il = pos / PPI;
    return stage1_at(pos, il, pos - il * PPI - 2);
  };
  // B fragment of the conv1 output row whose input rows are at positions pos .. pos + 4
  // (pos is wave-uniform: its ring row is a scalar, and a lane's row 0 .. 4 further on wraps
  // at most once: offset o < 2 RB is o mod RB = min(o, o - RB) in unsigned arithmetic)
  auto bfrag = [&](int pos) -> uint4 {
    constexpr uint32_t RB = E2R1 * C1ROW * 4;
    const uint32_t sb = (uint32_t)(pos & (E2R1 - 1)) * (C1ROW * 4);
    const uint32_t oA = sb + boA, oK = sb + boK;
    const unsigned char* r1b = reinterpret_cast<const unsigned char*>(ring1);
    return c1_bfrag(reinterpret_cast<const uint32_t*>(r1b + min(oA, oA - RB)),
                    reinterpret_cast<const uint32_t*>(r1b + min(oK, oK - RB)));
  };
  // the four accumulators of a pool window (rows dy of the two fragments x column parities),
  // bias + all 25 taps in one MFMA each, into the running max v (starts at 0: ReLU folded)
  auto c1_window = [&](float (&v)[4], const uint4& bA, const uint4& bB, const f32x4& bias1) {
#pragma unroll
    for (int pr = 0; pr < 4; ++pr) {
      const f32x4 acc1 = mfma16x16x32<T>(pr & 1 ? v1 : v0, pr >> 1 ? bB : bA, bias1);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], acc1[i]);
    }
  };
  // conv2 input row 2 q2 + jr of conv2 step g2 (image g2 / SPI) into its ring slot: pooled
  // pixels 16 w1x + m, channels 4 kg .. 4 kg + 3 (zero rows outside the image)
  auto produce = [&](int g2, int il, int q2) {  // g2 = il SPI + q2
    const int r = 2 * q2 + jr;
    // branch-free (the step stays one basic block, so the scheduler can interleave these
    // MFMAs with conv2's): rows past the image are computed from whatever finite rows the
    // ring holds and replaced by zeros
    const int pb = 4 * g2 + 2 * jr;  // position of image row 2r - 2
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const uint4 bA = bfrag(pb), bB = bfrag(pb + 1);
    c1_window(v, bA, bB, *reinterpret_cast<const f32x4*>(btab + 4 * kg));
    const bool real = il < nimg && r < H;
    const uint2 pk = real ? uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])} : uint2{0u, 0u};
    *reinterpret_cast<uint2*>(ring + ((2 * g2 + jr) & 7) * C::ROWB + (16 * w1x + m + 2) * 32 +
                              8 * kg) = pk;
  };

  __syncthreads();  // rings zeroed
  for (int pp = 0; pp < 32; pp += 4) stage1(pp);  // positions 0 .. 31 (steps -8 .. -1)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  lds_barrier();
  produce(0, 0, 0);
  produce(1, 1 / SPI, 1 % SPI);
  lds_barrier();

  f32x4 acc[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = bias2_ld();
  T* __restrict__ O = reinterpret_cast<T*>(a.out);
  const int PW = 32, PHh = H / 2;
  int c_1 = 0, c_2 = 0;  // this wave's vector-memory ops (store + LDS-DMA) of steps s - 1, s - 2
  // scalar counters: steps s - 2 (pool), s (conv2), s + 2 (conv1) as (image, step in image),
  // and this wave's stage-1 position 4 s + 32 + wv as (image, row); floor division once here
  auto fdiv = [](int x, int d) { return x >= 0 ? x / d : -((-x + d - 1) / d); };
  int ilA = fdiv(-2, SPI), qA = -2 - ilA * SPI;
  int qC = 0;
  int ilB = 2 / SPI, qB = 2 - ilB * SPI;
  int ilD = (32 + wv) / PPI, rD = 32 + wv - ilD * PPI;  // row y = rD - 2
  auto adv = [](int& il, int& q, int by, int per) {
    q += by;
    if (q >= per) { q -= per; ++il; }
  };
#ifdef SPECENH_CR_STATS
  CRClock clk;
#endif

  if constexpr (SCHED == 1) {
    // ---- schedule 1 (header comment) ----
    unsigned char* const tile = lds + E2LDS;
    unsigned char* const tw = tile + e2_tile_write((x0 + m) >> 1, 4 * nb + kg);
    // (waves 6, 7; formed where used: two registers fewer to keep through the loop)
    auto store_tile = [&](unsigned char* base, int tb) {
      int l = lane;
      asm volatile("" : "+v"(l));
      const uint4 v = *reinterpret_cast<const uint4*>(tile + tb + e2_tile_read(wv & 1, l));
      gstore16_s<0>(base, 1024u * (wv & 1) + 16u * l, v);
    };
    // (values that a run-time division made on the VALU, into scalar registers for good)
    const int nimgs = __builtin_amdgcn_readfirstlane(nimg);
    ilD = __builtin_amdgcn_readfirstlane(ilD);
    rD = __builtin_amdgcn_readfirstlane(rD);
    // What a step's branches and selects ask is a property of a position of the workgroup's
    // step stream (step t = il SPI + q: image il, pair q; q = SPI - 1 = PHh is the bubble)
    // looked at from three distances: conv1 works for t = s + 2, conv2 on t = s, the pool on
    // t = s - 2, the tile store on t = s - 3. So the stream is walked once, two steps ahead,
    // and three bits per position are shifted through one word: E2F_REAL the pair is inside
    // an image of this workgroup, E2F_BUB it is a bubble, E2F_TOP it is an image's first.
    // Position t's bits sit 3 (s + 2 - t) places up. (restated in
    // tests/test_enc2_stage_mapping.py)
    constexpr unsigned E2F_REAL = 1u, E2F_BUB = 2u, E2F_TOP = 4u;
    constexpr unsigned F_PROD = E2F_REAL, F_CBUB = E2F_BUB << 6, F_CTOP = E2F_TOP << 6,
                       F_OTOP = E2F_TOP << 12, F_HELD = E2F_REAL << 15;
    int ilT = 0, qT = 0;  // position s + 2
    unsigned fl = 0;
    // (a < b as the difference's sign bit: see conv_rows_pool_kernel's schedule 1)
    auto lt = [](int x, int y) -> unsigned { return (unsigned)(x - y) >> 31; };
    auto push = [&]() {  // position (ilT, qT) into the word (qT <= PHh)
      const unsigned in = lt(qT, PHh);
      fl = (fl << 3) | ((lt(ilT, nimgs) & in) * E2F_REAL) | ((in ^ 1u) * E2F_BUB) |
           (lt(qT, 1) * E2F_TOP);
    };
    auto walk = [&]() {
      if (++qT == SPI) { qT = 0; ++ilT; }
    };
    push();  // t = 0 .. 2 (the positions before the stream are no pairs: zeros)
    walk();
    push();
    walk();
    push();
    fl = __builtin_amdgcn_readfirstlane(fl);
    // the pooled row of pair t: its 2 KB at ob, the next pair's one row on, the next image's
    // first (n -> n + G) a constant jump from the row past an image's last. ob is pair
    // s - 2's, obp pair s - 3's. It starts at pair SPI - 2 of the image one grid before the
    // workgroup's first (a position of the walk, never stored to), so that the jump into
    // position 0 is the same as every later one
    constexpr long long ROWO = E2TILE;
    unsigned char* ob = reinterpret_cast<unsigned char*>(a.out) +
                        (((long long)blockIdx.x - G) * PHh + SPI - 2) * ROWO;
    unsigned char* obp = ob - ROWO;
    const long long ojump = (long long)(G - 1) * PHh * ROWO;
    // this wave's image row of the DMA (row rD - 2 of image ilD: outside the image at rD = zr,
    // the first of waves 0, 1 and the last of waves 2, 3), four rows on per step. Like ob it is
    // a position of the walk: it points outside the tensor whenever dreal is 0 (rows -2, -1,
    // H1, H1 + 1 and the images past the workgroup's last) and is not dereferenced then
    constexpr long long ROWX = (long long)C1W * (long long)sizeof(T);
    const unsigned char* xs = reinterpret_cast<const unsigned char*>(a.x) +
        (((long long)blockIdx.x + (long long)ilD * G) * H1 + rD - 2) * ROWX;
    const long long xjump = (long long)(G - 1) * H1 * ROWX;
    const int zr = wv < 2 ? wv : H1 + wv;
    auto dma_real = [&]() { return lt(ilD, nimgs) & (lt(rD, zr) | lt(zr, rD)); };
    unsigned dreal = __builtin_amdgcn_readfirstlane(dma_real());
    // step s + 1's positions, pointers and flags, computed under step s's MFMAs and pinned
    // there by the empty asm: a step opens with tests of bits
    auto next = [&]() {
      walk();
      push();
      obp = ob;
      ob += (fl & F_OTOP) ? ojump : ROWO;
      rD += 4;
      if (rD >= PPI) { rD -= PPI; ++ilD; xs += xjump; } else { xs += 4 * ROWX; }
      dreal = __builtin_amdgcn_readfirstlane(dma_real());
      fl = __builtin_amdgcn_readfirstlane(fl);
      asm volatile("" : "+s"(fl), "+s"(dreal), "+s"(ob), "+s"(obp), "+s"(xs));
    };
    auto ld16 = [](const unsigned char* p) { return *reinterpret_cast<const uint4*>(p); };
    // (conv1's running max of the window's four outputs, c1_window, is schedule 0's: it compiles
    // to two v_max3_f32 per value; on packed pairs it took as many instructions, with the
    // converts, and more registers)

    auto step1 = [&](auto ic, const int s) {
      constexpr int I = decltype(ic)::value % 3, P = decltype(ic)::value & 1;
      auto slot = [](int d) { return (2 * I + d + 12) % 6; };
      const unsigned flc = fl;  // this step's flags (next() below makes step s + 1's)
      f32x4& r0 = acc[slot(-4)];
      f32x4& r1 = acc[slot(-3)];
      // (1) the pooled row that step s - 1 left in its tile: two whole-line stores
      if (wv >= 6 && (flc & F_HELD)) store_tile(obp, (P ^ 1) * E2TILE);
      CR_MARK(0);
      // (2) image rows 8 steps ahead (as schedule 0)
      int nd = 0;
      if (wv < 4) {
        uint32_t* dst = ring1 + ((4 * s + wv) & (E2R1 - 1)) * C1ROW + 4;
        if (dreal) {
          if (lane < 16) lds_dma16_s(xs, 16u * lane, dst);
          nd = 1;
        } else {
          int z = 0;
          asm volatile("" : "+v"(z));
          if (lane < 16) *reinterpret_cast<uint4*>(dst + 4 * lane) = uint4{(uint32_t)z, (uint32_t)z, (uint32_t)z, (uint32_t)z};
        }
      }
      CR_MARK(1);
      // (3) the arithmetic, opened by conv1's two B fragments (the window rows of step s + 2:
      // eight ds_read_b32 in flight at once). conv2's input rows (2s, 2s + 1: ring slots rs,
      // rs + 1, rs even) landed before the barrier. The F fragment of the bubble's
      // second row and F(-1) off an image's top are read from the ring's first 16 bytes, a
      // halo no step writes (zeros), by address select; F(-1) only in lane groups 2, 3.
      const int rs = (2 * s) & 7;
      const unsigned char* rb = ring + rs * C::ROWB;
      const int pb = 4 * (s + 2) + 2 * jr;
      const uint4 bA = bfrag(pb), bB = bfrag(pb + 1);
      // (slot 7 pairs with slot 0: foffw = foff - 8 ROWB in lane groups 2, 3)
      const int fo1 = (flc & F_CBUB) ? 0 : (rs + 1) * C::ROWB + (rs == 6 && kg >= 2 ? foff - 8 * C::ROWB : foff);
      const int foT = (flc & F_CTOP) && kg >= 2 ? (rs - 1) * C::ROWB + foff : 0;  // (fo = foff - ROWB there)
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      auto c2 = [&](int j, int w, const uint4& b) {  // weight fragment w of row j: its output row
        const int d = w < 10 ? j + 2 - w % 5 : w == 10 ? j + 2 : w == 11 ? j : j - 2;
        acc[slot(d)] = mfma16x16x32<T>(wf[w], b, acc[slot(d)]);
      };
      {  // pair s - 2: pool on the packed pairs (rows in lane, columns across the lane pair
         // m, m ^ 1, ReLU), reset, into the tile: unconditionally, a tile no flag marks is
         // never stored
        auto nbr = [](uint32_t x) {
          return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);
        };
        const uint32_t p0 = max_s16x2(pack2_cvt<T>(r0[0], r0[1]), pack2_cvt<T>(r1[0], r1[1]));
        const uint32_t p1 = max_s16x2(pack2_cvt<T>(r0[2], r0[3]), pack2_cvt<T>(r1[2], r1[3]));
        const f32x4 bias = bias2_ld();
        r0 = bias;
        r1 = bias;
        *reinterpret_cast<uint2*>(tw + P * E2TILE) =
            uint2{max_s16x2(max_s16x2(p0, nbr(p0)), 0u), max_s16x2(max_s16x2(p1, nbr(p1)), 0u)};
      }
      next();
      c1_window(v, bA, bB, *reinterpret_cast<const f32x4*>(btab + 4 * kg));
      CR_MARK(2);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const unsigned char* rbj = rb + j * C::ROWB;
        const uint4 b0 = ld16(rbj + boff), b2 = ld16(rbj + boff + 64);
        const uint4 bF = j ? ld16(ring + fo1) : ld16(rbj + foff);
#pragma unroll
        for (int w = 0; w < 5; ++w) c2(j, w, b0);
#pragma unroll
        for (int w = 5; w < 10; ++w) c2(j, w, b2);
        c2(j, 10, bF); c2(j, 11, bF); c2(j, 12, bF);
        if (j == 0) acc[slot(1)] = mfma16x16x32<T>(wf[10], ld16(ring + foT), acc[slot(1)]);
      }
      // conv2 input row 2 q + jr of step s + 2 into its ring slot (zeros outside the image)
      {
        const uint2 pv = uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])};
        const uint32_t keep = 0u - (flc & F_PROD);
        *reinterpret_cast<uint2*>(ring + ((2 * s + 4 + jr) & 7) * C::ROWB + (16 * w1x + m + 2) * 32 +
                                  8 * kg) = uint2{pv.x & keep, pv.y & keep};
      }
      CR_MARK(3);
      // (4) the DMA of step s - 3 has landed: wait for all but the DMAs issued after it (the
      // DMA waves issue nothing else)
      if (wv < 4) wait_vmcnt_ss<3>(c_2 + c_1 + nd);
      c_2 = c_1;
      c_1 = nd;
      CR_MARK(4);
      lds_barrier();
      CR_MARK(5);
    };
    const int Ss = __builtin_amdgcn_readfirstlane(S);
    CR_MARK(-1);
    for (int s = 0; s < Ss; s += 6) {
      step1(std::integral_constant<int, 0>{}, s);
      if (s + 1 >= Ss) break;
      step1(std::integral_constant<int, 1>{}, s + 1);
      if (s + 2 >= Ss) break;
      step1(std::integral_constant<int, 2>{}, s + 2);
      if (s + 3 >= Ss) break;
      step1(std::integral_constant<int, 3>{}, s + 3);
      if (s + 4 >= Ss) break;
      step1(std::integral_constant<int, 4>{}, s + 4);
      if (s + 5 >= Ss) break;
      step1(std::integral_constant<int, 5>{}, s + 5);
    }
    // the last step's pooled row (the barrier that ended it published the tile)
    if (wv >= 6 && (fl & F_HELD)) store_tile(obp, ((Ss - 1) & 1) * E2TILE);
#ifdef SPECENH_CR_STATS
    clk.flush(wv);
#endif
    return;
  }

  auto step = [&](auto ic, const int s) {
    constexpr int I = decltype(ic)::value;
    auto slot = [](int d) { return (2 * I + d + 12) % 6; };
    int ns = 0;  // stores issued by this wave in this step
    {  // conv2 pair s - 2: pool, store, reset
      f32x4& r0 = acc[slot(-4)];
      f32x4& r1 = acc[slot(-3)];
      {
        const int il = ilA, q = qA;
        if (il >= 0 && il < nimg && q < PHh) {
          ns = 1;
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = fmaxf(max_pair(fmaxf(r0[i], r1[i])), 0.f);
          // lanes m and m ^ 1 hold the same pooled values (max_pair) and store them to the same
          // pixel: no exec-mask branch around the store
          const long long n = (long long)blockIdx.x + (long long)il * G;
          const long long o = ((n * PHh + q) * PW + (x0 + m) / 2) * 32 + 16 * nb + 4 * kg;
          *reinterpret_cast<uint2*>(O + o) = uint2{pack2_cvt<T>(v[0], v[1]), pack2_cvt<T>(v[2], v[3])};
        }
      }
      const f32x4 bias = bias2_ld();
      r0 = bias;
      r1 = bias;
    }
    CR_MARK(0);
    // image rows 8 steps ahead (positions 4s + 32 .. 4s + 35: slots of 4s .. 4s + 3, whose
    // last readers were this step's predecessors), conv2 input rows of step s + 2 (positions
    // 4s + 8 .. 4s + 15: DMAs of steps s - 6 and s - 5, waited at the end of step s - 2)
    const int nd = wv < 4 ? stage1_at(4 * s + 32 + wv, ilD, rD - 2) : 0;
    CR_MARK(1);
    // this step's conv2 rows, unconditionally: past an image they are the zero rows the
    // conv1 stage stored (adding nothing)
    const int q = qC;
    auto conv2_rows = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int rs = (2 * s + j) & 7;
      const unsigned char* rb = ring + rs * C::ROWB;
      const uint4 b0 = *reinterpret_cast<const uint4*>(rb + boff);
      const uint4 b2 = *reinterpret_cast<const uint4*>(rb + boff + 64);
      uint4 bF = *reinterpret_cast<const uint4*>(rb + (rs == 7 ? foffw : foff));
      // the bubble step's F(H + 1) would pair the zero row H + 1 with the NEXT image's row 0
      // (the next ring slot) and add it to that image's output rows 1 / -1 (pair s + 1 is
      // the next image's rows 0, 1): zero it (the next image's F(-1) adds that term)
      if (j == 1 && q == SPI - 1) bF = uint4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int ky = 0; ky < 5; ++ky) {
        f32x4& ac = acc[slot(j + 2 - ky)];
        ac = mfma16x16x32<T>(wf[ky], b0, ac);
      }
#pragma unroll
      for (int ky = 0; ky < 5; ++ky) {
        f32x4& ac = acc[slot(j + 2 - ky)];
        ac = mfma16x16x32<T>(wf[5 + ky], b2, ac);
      }
      acc[slot(j + 2)] = mfma16x16x32<T>(wf[10], bF, acc[slot(j + 2)]);
      acc[slot(j)] = mfma16x16x32<T>(wf[11], bF, acc[slot(j)]);
      acc[slot(j - 2)] = mfma16x16x32<T>(wf[12], bF, acc[slot(j - 2)]);
      if (j == 0) {  // F(-1) at the top of an image (q == 0), zero otherwise
        uint4 bT = *reinterpret_cast<const uint4*>(ring + ((2 * s) & 7) * C::ROWB + fo);
        if (kg < 2 || q != 0) bT = uint4{0u, 0u, 0u, 0u};
        acc[slot(1)] = mfma16x16x32<T>(wf[10], bT, acc[slot(1)]);
      }
    }
    };
    // The two waves of a SIMD (w, w + 4) run the same program and meet at one barrier per
    // step; run in the same order, both would read conv1's LDS-heavy B fragments, then both
    // issue conv2's MFMAs. Waves 4-7 take the two halves in the other order (they are
    // independent: produce writes the ring slots of step s + 2, conv2 reads those of steps s,
    // s + 1), so each SIMD pairs one wave's conv1 with the other's conv2 (MI355X_MICROARCH.md,
    // two waves per SIMD, item 9: a stagger). Measured slower (0.337 vs 0.311 ms per 2048,
    // profiles/r05_enc2_stagger_ab.txt; its VGPR spills rose 5 -> 20), so off by default.
    if (SPECENH_ENC2_STAGGER && wv >= 4) {
      conv2_rows();
      produce(s + 2, ilB, qB);
    } else {
      produce(s + 2, ilB, qB);
      CR_MARK(2);
      conv2_rows();
    }
    CR_MARK(3);
    // the DMA of step s - 3 (first read by conv1 at step s + 2) must have landed: wait for all
    // but this wave's vector-memory ops of steps s - 2 .. s (each step: its store, then its
    // DMA). Only the DMA waves wait; stores alone are never waited for.
    if (wv < 4) {
      const int younger = c_2 + c_1 + ns + nd;
      if (younger >= 6) {  // (steady state: store + DMA in each of the three steps)
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      } else switch (younger) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      }
    }
    c_2 = c_1;
    c_1 = ns + nd;
    adv(ilA, qA, 1, SPI);
    qC = qC + 1 == SPI ? 0 : qC + 1;
    adv(ilB, qB, 1, SPI);
    adv(ilD, rD, 4, PPI);
    CR_MARK(4);
    lds_barrier();
    CR_MARK(5);
  };
  CR_MARK(-1);
  int s = 0;
  for (; s + 3 <= S; s += 3) {
    step(std::integral_constant<int, 0>{}, s);
    step(std::integral_constant<int, 1>{}, s + 1);
    step(std::integral_constant<int, 2>{}, s + 2);
  }
  if (s < S) step(std::integral_constant<int, 0>{}, s);
  if (s + 1 < S) step(std::integral_constant<int, 1>{}, s + 1);
#ifdef SPECENH_CR_STATS
  clk.flush(wv);
#endif
}

template <typename T, int WPE, int SCHED>
hipError_t launch_enc2_wpe(const E2Args& a, hipStream_t st) {
  constexpr int LDSB = SCHED == 1 ? E2LDS1 : E2LDS;
  const void* k = reinterpret_cast<const void*>(&enc2_rows_kernel<T, WPE, SCHED>);
  static ResidentSlots site;
  long long slots = 0;
  const hipError_t e = resident_slots(site, k, 512, LDSB, &slots);
  if (e != hipSuccess) return e;
  const long long grid = std::min<long long>(a.N, slots);
  SPECENH_LAUNCH((enc2_rows_kernel<T, WPE, SCHED>), dim3((unsigned)grid), dim3(512), LDSB, st, a);
  return hipGetLastError();
}

// schedule 1 (variant ENC2_SCHED, the default) for the two-workgroups-per-CU build when the
// output is 16-byte aligned (its whole-line stores are 16 bytes per lane); the earlier step
// otherwise
template <typename T>
hipError_t launch_enc2(const E2Args& a, hipStream_t st) {
  if (variant(V_ENC2_WPE2)) return launch_enc2_wpe<T, 2, 0>(a, st);
  if (variant(V_ENC2_SCHED) != 0 && ((uintptr_t)a.out & 15) == 0) return launch_enc2_wpe<T, 4, 1>(a, st);
  return launch_enc2_wpe<T, 4, 0>(a, st);
}

// an entry's result from its launch's: *launched on success, the HIP error under `what` otherwise
int rows_result(hipError_t e, const char* what, bool* launched) {
  if (e != hipSuccess) return set_error(SPECENH_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  *launched = true;
  return SPECENH_OK;
}

}  // namespace

// The row-sweep kernel for an inference Conv2D(5, relu, same) + MaxPooling2D(2) when the
// shape is one it is built for; *launched = false otherwise (the caller runs
// conv_patch_kernel).
int conv_rows_pool(int dtype, const void* x, int N, int H, int W, int CI, const void* w,
                   const float* b, int CO, int K, void* out, hipStream_t st, bool* launched) {
  *launched = false;
  if (variant(V_CONV_NO_ROWS) != 0 || N <= 0 || H < 2 || (H & 1) || !b) return SPECENH_OK;
  if ((long long)N * H * W * CI >= (1ll << 31)) return SPECENH_OK;
  if (dtype != SPECENH_DTYPE_F16 && dtype != SPECENH_DTYPE_BF16) return SPECENH_OK;
  const CRArgs a{x, w, b, out, N, H, 0};
  const bool k5 = K == 5, covered = (CI == 16 && CO == 32 && W == 64 && k5) ||
                                    (CI == 32 && CO == 64 && W == 32 && k5) ||
                                    (CI == 32 && CO == 32 && W == 64 && (k5 || K == 3));
  if (!covered) return SPECENH_OK;
  const hipError_t e = with_half_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (CI == 16) return launch_rows<T, 16, 32, 64>(a, st);
    if (CO == 64) return variant(V_CONV_ROWS_SCHED) != 0 ? launch_rows<T, 32, 64, 32, 5, 1>(a, st)
                                                         : launch_rows<T, 32, 64, 32>(a, st);
    // hyperparam_scan.py, 256 x 128 inputs
    return k5 ? launch_rows<T, 32, 32, 64>(a, st) : launch_rows<T, 32, 32, 64, 3>(a, st);
  });
  return rows_result(e, "conv_rows", launched);
}

// The row-sweep kernel for Conv2DTranspose(CO, 5, s2, relu, same) on 64-channel inputs of
// width 16 (CO 64) or 32 (CO 32), forward (any batch); *launched = false otherwise.
int convt_rows(int dtype, const void* x, int N, int H, int W, int CI, const void* w,
               const float* b, int CO, int K, void* out, hipStream_t st, bool* launched) {
  *launched = false;
  if (variant(V_CONVT_NO_ROWS) != 0 || N <= 0 || H <= 0 || !b) return SPECENH_OK;
  if (dtype != SPECENH_DTYPE_F16 && dtype != SPECENH_DTYPE_BF16) return SPECENH_OK;
  if ((long long)N * 4 * H * W * CO >= (1ll << 31)) return SPECENH_OK;
  const CRArgs a{x, w, b, out, N, H, 0};
  if (CI == 32) {  // the scan models' first Conv2DTranspose (32 -> 32 on 32-position rows)
    if (CO != 32 || W != 32 || (K != 3 && K != 5 && K != 7)) return SPECENH_OK;
    const hipError_t e = with_half_type(dtype, [&](auto t) {
      using T = decltype(t);
      return K == 3   ? launch_convt_rows32<T, 32, 32, 3>(a, st)
             : K == 5 ? launch_convt_rows32<T, 32, 32, 5>(a, st)
                      : launch_convt_rows32<T, 32, 32, 7>(a, st);
    });
    return rows_result(e, "convt_rows32", launched);
  }
  if (CI != 64 || K != 5 || !((CO == 64 && W == 16) || (CO == 32 && W == 32))) return SPECENH_OK;
  const hipError_t e = with_half_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (CO == 32) return launch_convt_rows<T, 32, 32>(a, st);
    if (variant(V_CONVT_SHARED_RING) != 0) return launch_convt_rows<T, 64, 16>(a, st);
    if (variant(V_CONVT_PG) != 0) return launch_convt_rows_pg<T>(a, st);
    return variant(V_CONVT_STORE8) != 0 ? launch_convt_rows_pw<T, true>(a, st)
                                        : launch_convt_rows_pw<T, false>(a, st);
  });
  return rows_result(e, "convt_rows", launched);
}

// The C = 1 row sweep for an inference Conv2D(16, 5, relu, same) + MaxPooling2D(2) on
// 128-wide images; *launched = false otherwise (the caller runs conv_c1_mfma).
int conv1_rows_pool(int dtype, const void* x, int N, int H, int W, const void* w,
                    const float* b, int CO, void* out, hipStream_t st, bool* launched) {
  *launched = false;
  if (variant(V_CONV1_NO_ROWS) != 0 || N <= 0 || H < 2 || (H & 1) || W != C1W || CO != 16 || !b)
    return SPECENH_OK;
  if (dtype != SPECENH_DTYPE_F16 && dtype != SPECENH_DTYPE_BF16) return SPECENH_OK;
  if (((uintptr_t)x & 15) || (long long)N * H * W >= (1ll << 31)) return SPECENH_OK;
  const CRArgs a{x, w, b, out, N, H, 0};
  const hipError_t e =
      with_half_type(dtype, [&](auto t) { return launch_conv1_rows<decltype(t)>(a, st); });
  return rows_result(e, "conv1_rows", launched);
}

}  // namespace specenh

// Conv2D(16, 5, relu, same) + MaxPooling2D(2) + Conv2D(32, 5, relu, same) + MaxPooling2D(2)
// on [N][H][128][1] 16-bit images (H a multiple of 4) in one launch (enc2_rows_kernel).
extern "C" int specenh_encoder2(int dtype, const void* x, int N, int H, int W, const void* w1_gemm,
                                const float* b1, int CO1, const void* w2_gemm, const float* b2,
                                int CO2, int k, void* out, void* stream) {
  using namespace specenh;
  if (N < 0 || H <= 0 || W <= 0) return set_error(SPECENH_EINVAL, "bad input shape");
  if (dtype != SPECENH_DTYPE_F16 && dtype != SPECENH_DTYPE_BF16)
    return set_error(SPECENH_EUNSUPPORTED, "fused encoder: fp16 / bf16 only");
  if (W != C1W || CO1 != 16 || CO2 != 32 || k != 5 || (H & 3))
    return set_error(SPECENH_EUNSUPPORTED,
                     "fused encoder: Conv2D(16, 5) + pool + Conv2D(32, 5) + pool on 128-wide "
                     "one-channel images, height a multiple of 4");
  if (N == 0) return SPECENH_OK;
  if (!x || !w1_gemm || !b1 || !w2_gemm || !b2 || !out) return set_error(SPECENH_EINVAL, "null pointer");
  if (((uintptr_t)x & 15) || (long long)N * H * W >= (1ll << 31))
    return set_error(SPECENH_EINVAL, "input must be 16-byte aligned and below 2^31 elements");
  E2Args a{};
  a.x = x; a.w1 = w1_gemm; a.b1 = b1; a.w2 = w2_gemm; a.b2 = b2; a.out = out; a.N = N; a.H = H;
  hipStream_t st = (hipStream_t)stream;
  static LdsOptIn lds_site;
  hipError_t e = allow_lds(lds_site,
                           {reinterpret_cast<const void*>(&enc2_rows_kernel<_Float16, 4, 1>),
                            reinterpret_cast<const void*>(&enc2_rows_kernel<__bf16, 4, 1>),
                            reinterpret_cast<const void*>(&enc2_rows_kernel<_Float16, 4, 0>),
                            reinterpret_cast<const void*>(&enc2_rows_kernel<__bf16, 4, 0>),
                            reinterpret_cast<const void*>(&enc2_rows_kernel<_Float16, 2, 0>),
                            reinterpret_cast<const void*>(&enc2_rows_kernel<__bf16, 2, 0>)},
                           E2LDS1);
  if (e == hipSuccess)
    e = with_half_type(dtype, [&](auto t) { return launch_enc2<decltype(t)>(a, st); });
  if (e != hipSuccess) return set_error(SPECENH_EHIP, std::string("encoder2: ") + hipGetErrorString(e));
  return SPECENH_OK;
}

#ifdef SPECENH_CR_STATS
extern "C" int specenh_cr_stats(void* host, int bytes) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(specenh::cr_stats), bytes) == hipSuccess ? 0 : -1;
}
#endif
