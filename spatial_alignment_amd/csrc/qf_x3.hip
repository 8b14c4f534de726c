// panel_elbo_x3_kernel: panel_elbo_kernel (qf_elbo.hip) with its contraction W_l = Omega_l alpha done on the bf16
// matrix instructions in three pieces (the opt-in contraction mode gpsa_step_desc.contraction = 1).
//
// Every fp32 operand is written as a = a1 + a2 + a3, each piece the bf16 rounding of what the earlier ones left
// (8 + 8 + 8 significant bits); the six products a_i b_j with i + j <= 4 carry everything above 2^-24 |a b|, each is
// exact in the accumulator's product stage, and the accumulation is the same fp32 one the fp32 instruction does.  Per
// 32 k: six v_mfma_f32_16x16x32_bf16 (16 cycles each) against eight v_mfma_f32_16x16x4_f32 (32 cycles each).
// The experiment behind it is split_bf16.hip (tools/split_bf16_parity.py, LAB_NOTES).
//
// K order.  A K block is 32 rows of alpha = row tiles 2b and 2b + 1.  Lane (j, kq) of the B operand holds eight k
// values; they are chosen as rows 4 kq .. 4 kq + 3 of tile 2b, then of tile 2b + 1 - exactly the rows the lane's
// accumulators hold for those tiles (C/D layout: lane (j, kq) holds rows 4 kq .. + 3 of column j).  The packer orders
// Omega's columns the same way (the MFMA sums over k: a permutation applied to both operands is free), so the closing's
// v = alpha . W reads alpha from the lane's own B pieces, rebuilt as (a1 + a2) + a3 - bit-equal to the fp32 alpha
// (the two differences of the split are exact) - and no fp32 copy of the slab is kept.
//
// Schedule: panel_elbo_kernel's (persistent balanced items, TileOrder, LDS-DMA ring, register-resident alpha slab,
// same closing, slabs and partial sums).  A ring slot is one K block of all row tiles in three planes, MB x 3 KiB
// (39 KiB at MB = 13; a slot is NPW * 4 = 40 pieces with the surplus ones, so the ring takes 120 KiB of the 160 KiB)
// with two stages in flight; a fourth slot does not fit at MB = 16, and the three-slot ring already has a whole K block
// of MFMAs (13 row tiles x 6 = 78 at NCT = 1) between a stage's issue and its use.
#include "qf_common.hpp"

namespace gpsa {

typedef __bf16 x3_bf16x8 __attribute__((ext_vector_type(8)));

// x[0..7] -> three bf16 pieces (round to nearest even), x = p0 + p1 + p2 up to subnormals
__device__ __forceinline__ void x3_split(const float (&x)[8], x3_bf16x8 (&p)[3]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const __bf16 h0 = (__bf16)x[e];
    float r = x[e] - (float)h0;
    const __bf16 h1 = (__bf16)r;
    r -= (float)h1;
    p[0][e] = h0;
    p[1][e] = h1;
    p[2][e] = (__bf16)r;
  }
}

// column of Omega (= row of alpha) of element e of lane group kq in K block b
__host__ __device__ __forceinline__ int x3_kidx(int b, int kq, int e) { return 32 * b + (e < 4 ? 4 * kq + e : 16 + 4 * kq + e - 4); }

// Omega -> [L][KB][MB][3][64 lanes][8] bf16: piece (l, b, rt, plane) is the A fragment of row tile rt in K block b,
// lane i + 16 kq holding Omega[16 rt + i][x3_kidx(b, kq, 0..7)].  The fp32 rounding of Omega is what gets split (the
// only difference from the fp32 path is then the contraction); row M carries delta[:, l] when drow is given (the
// delta-in-padding-row form, as pack_panels_kernel).  One thread per (l, b, rt, lane).
template <typename TS>
__global__ void __launch_bounds__(256) pack_x3_kernel(const TS* __restrict__ src, int M, int MB, int KB, int L,
                                                       unsigned short* __restrict__ dst, const float* __restrict__ drow) {
  const long long idx = blockIdx.x * 256LL + threadIdx.x;
  const long long per = (long long)KB * MB * 64;
  if (idx >= per * L) return;
  const int l = (int)(idx / per);
  const int rem = (int)(idx % per);
  const int b = rem / (MB * 64), rt = (rem / 64) % MB, lane = rem % 64;
  const int i = rt * 16 + (lane & 15), kq = lane >> 4;
  const TS* sp = src + (long long)l * M * M;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = x3_kidx(b, kq, e);
    float x = 0.f;
    if (i < M && k < M) x = (float)sp[(long long)i * M + k];
    else if (drow != nullptr && i == M && k < M) x = drow[(long long)k * L + l];
    v[e] = x;
  }
  x3_bf16x8 p[3];
  x3_split(v, p);
  x3_bf16x8* out = reinterpret_cast<x3_bf16x8*>(dst) + (((long long)l * KB + b) * MB + rt) * 3 * 64 + lane;
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q * 64] = p[q];
}
template __global__ void pack_x3_kernel<float>(const float* __restrict__, int, int, int, int, unsigned short* __restrict__,
                                               const float* __restrict__);
template __global__ void pack_x3_kernel<double>(const double* __restrict__, int, int, int, int, unsigned short* __restrict__,
                                                const float* __restrict__);

template <int MB, int NCT>
__global__ void __launch_bounds__(256, 1) panel_elbo_x3_kernel(ElboArgs a) {
  constexpr int MP = MB * 16;
  constexpr int KB = (MB + 1) / 2;           // 32-deep K blocks (the last one half empty when MB is odd)
  constexpr int WGCOLS = 64 * NCT;
  constexpr int NPIECE = MB * 3;             // 1-KiB pieces of a chunk (one K block of every row tile, three planes)
  constexpr int NPW = (NPIECE + 3) / 4;      // LDS-DMA operations per wave and stage (uniform: surplus pieces repeat)
  constexpr int CHUNK = NPIECE * 512;        // bf16 of one chunk
  constexpr int NGATHER = (3 * NCT * 16 + 63) / 64;
  constexpr int NSLOT = 3, AHEAD = 2;
  __shared__ __attribute__((aligned(16))) unsigned short lds[NSLOT][NPW * 4 * 512];
  __shared__ __attribute__((aligned(16))) float sgat[4][NGATHER * 64];
  __shared__ double red[4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const unsigned short* __restrict__ Ppk = reinterpret_cast<const unsigned short*>(a.Ppk);
  const float* __restrict__ X = a.X;
  const int M = a.M, L = a.L;
  const long long C = a.C;

  const long long ntiles = (C + WGCOLS - 1) / WGCOLS;
  const long long T = ntiles * L;
  const long long it0 = (long long)blockIdx.x * T / gridDim.x;
  const long long it1 = (long long)(blockIdx.x + 1) * T / gridDim.x;
  if (blockIdx.x == 0)
    for (int i = (int)gridDim.x + tid; i < a.nparts; i += 256) a.part[i] = 0.0;
  if (it0 >= it1) {
    if (tid == 0) a.part[blockIdx.x] = 0.0;
    return;
  }

  x3_bf16x8 xp[NCT][KB][3];  // the alpha slab in three planes (B operand)
  f32x4 acc[MB][NCT], ab[MB][NCT];
  const TileOrder ord(it0, it1, L);
  // stage cursor (as panel_elbo_kernel): the chunks of a step are consecutive in the packed operand
  long long sstep = 0, stile_;
  int sa_, sb_;
  ord.get(0, stile_, sa_, sb_);
  const unsigned short* sp = Ppk + (long long)sa_ * KB * CHUNK;
  int srem = (sb_ - sa_ + 1) * KB;
  // wave w stages pieces w, w + 4, ... of the chunk into the same positions of the slot; surplus ones re-load the last
  // piece into the slot's tail (never read).  Past the last chunk the cursor walks on behind it (up to AHEAD chunks:
  // the workspace holds the slabs there).
#define GPSA_X3_STAGE(BUF)                                                                             \
  {                                                                                                    \
    _Pragma("unroll") for (int pc = 0; pc < NPW; ++pc) {                                               \
      const int piece = pc * 4 + w;                                                                    \
      const unsigned short* src = sp + (piece < NPIECE ? piece : NPIECE - 1) * 512 + lane * 8;         \
      glds16(reinterpret_cast<const float*>(src), __builtin_amdgcn_readfirstlane(lds_addr(&lds[BUF][piece * 512]))); \
    }                                                                                                  \
    if (--srem > 0) {                                                                                  \
      sp += CHUNK;                                                                                     \
    } else if (sstep + 1 < ord.n) {                                                                    \
      ++sstep;                                                                                         \
      ord.get(sstep, stile_, sa_, sb_);                                                                \
      sp = Ppk + (long long)sa_ * KB * CHUNK;                                                          \
      srem = (sb_ - sa_ + 1) * KB;                                                                     \
    } else {                                                                                           \
      sp += CHUNK;                                                                                     \
      srem = 0x7fffffff;                                                                               \
    }                                                                                                  \
  }

  const double sN = exp((double)a.noise_u[0]) + 1e-5;
  const float inv = (float)(1.0 / sN);
  const float coef = (float)(-1.0 / (sN * sN * (double)a.S));
  const double var0 = exp((double)a.var_u[0]);
  double z2 = 0.0;

  int buf = 0;
  GPSA_X3_STAGE(0)
  GPSA_X3_STAGE(1)
  GPSA_DMA_WAIT(NPW);
  __syncthreads();

  for (long long step = 0; step < ord.n; ++step) {
    long long tile;
    int l_lo, l_hi;
    ord.get(step, tile, l_lo, l_hi);
    const long long cw = tile * WGCOLS + (long long)w * (16 * NCT);
    float resid[NCT];
    bool okc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      const long long c = cw + ct * 16 + j;
      okc[ct] = c < C;
      const long long cl = okc[ct] ? c : C - 1;
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int row = x3_kidx(b, kq, e);
          v[e] = X[(long long)(row < M ? row : M - 1) * C + cl];
          v[e] = (okc[ct] && row < M) ? v[e] : 0.f;
        }
        x3_split(v, xp[ct][b]);
      }
      const double qc = a.q[cl];
      resid[ct] = okc[ct] ? (float)(var0 - qc) : 1.f;
    }
    const float* gp[NGATHER];
    long long gstep[NGATHER];
#pragma unroll
    for (int o = 0; o < NGATHER; ++o) {
      int e = o * 64 + lane;
      if (e >= 3 * NCT * 16) e = 0;
      const int ct = e / 48, kind = (e % 48) / 16, jj = e % 16;
      long long c = cw + ct * 16 + jj;
      c = c < C ? c : C - 1;
      gp[o] = kind == 0 ? (a.meanT != nullptr ? a.meanT + (long long)l_lo * C + c : a.eps + c * L + l_lo)
                        : (kind == 1 ? a.eps + c * L + l_lo : a.Y + (c % a.N) * L + l_lo);
      gstep[o] = (kind == 0 && a.meanT != nullptr) ? C : 1;
    }
#pragma unroll
    for (int rt = 0; rt < MB; ++rt)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) asm("v_accvgpr_write_b32 %0, 0" : "=a"(ab[rt][ct][r]));
      }

    for (int l = l_lo; l <= l_hi; ++l) {
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        const int sbuf = buf + AHEAD >= NSLOT ? buf + AHEAD - NSLOT : buf + AHEAD;
        if (b == 0) {
          // this output's mean / eps / Y, ahead of the chunk's stage (the counted wait at its end then covers them)
          dma_set_m0(__builtin_amdgcn_readfirstlane(lds_addr(&sgat[w][0])));
          glds4_m0<0>(gp[0]);
          gp[0] += gstep[0];
          if (NGATHER > 1) {
            glds4_m0<256>(gp[NGATHER > 1 ? 1 : 0] - 64);
            gp[NGATHER > 1 ? 1 : 0] += gstep[NGATHER > 1 ? 1 : 0];
          }
          static_assert(NGATHER <= 2, "gather operations per wave and output");
        }
        const unsigned short* base = &lds[buf][lane * 8];
        x3_bf16x8 av[3], an[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) an[q] = *reinterpret_cast<const x3_bf16x8*>(base + q * 512);
#pragma unroll
        for (int rt = 0; rt < MB; ++rt) {
#pragma unroll
          for (int q = 0; q < 3; ++q) av[q] = an[q];
          if (rt + 1 < MB) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
              an[q] = *reinterpret_cast<const x3_bf16x8*>(base + ((rt + 1 < MB ? rt + 1 : 0) * 3 + q) * 512);
          }
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
            f32x4 c = b == 0 ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[rt][ct];
            // smallest products first
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[2], xp[ct][b][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], xp[ct][b][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], xp[ct][b][2], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[1], xp[ct][b][0], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], xp[ct][b][1], c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[0], xp[ct][b][0], c, 0, 0, 0);
            acc[rt][ct] = c;
          }
          __builtin_amdgcn_sched_barrier(0);  // (one row tile's fragments in flight: not the whole chunk's)
          if (rt == 0) {
            GPSA_X3_STAGE(sbuf)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
        // the next chunk has landed (all but the newest stage), and every wave is done with this slot
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        GPSA_DMA_WAIT(NPW);
        __syncthreads();
        buf = (buf == NSLOT - 1) ? 0 : buf + 1;
      }
      // closing of output l (panel_elbo_kernel's): alpha is rebuilt from its planes, (a1 + a2) + a3
      float z2l = 0.f;
      // (the rebuilt alpha is the same for every output: left to itself the compiler hoists it out of the output loop and
      //  keeps a second, fp32 copy of the slab live - the registers the split was meant to save)
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int b = 0; b < KB; ++b)
#pragma unroll
          for (int q = 0; q < 3; ++q) asm volatile("" : "+v"(xp[ct][b][q]));
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int rt = 0; rt < MB; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = (rt & 1) * 4 + r;
            const float x = ((float)xp[ct][rt >> 1][0][e] + (float)xp[ct][rt >> 1][1][e]) + (float)xp[ct][rt >> 1][2][e];
            if (r < 2) sa = fmaf(acc[rt][ct][r], x, sa);
            else sb = fmaf(acc[rt][ct][r], x, sb);
          }
        float s = sa + sb;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        float mean;
        if (a.meanT != nullptr) {
          mean = sgat[w][(ct * 3 + 0) * 16 + j];
        } else {
          const int lr = M - 16 * (MB - 1);
          const f32x4 t4 = acc[MB - 1][ct];
          const int r0 = lr & 3;
          const float pick = r0 == 0 ? t4.x : (r0 == 1 ? t4.y : (r0 == 2 ? t4.z : t4.w));
          mean = __shfl(pick, j + 16 * (lr >> 2), 64);
        }
        const float e = sgat[w][(ct * 3 + 1) * 16 + j];
        const float y = sgat[w][(ct * 3 + 2) * 16 + j];
        const float var = resid[ct] + s + 2e-5f;
        const float sd = sqrtf(var);
        const float Fd = mean + sd * e;
        const float rres = y - Fd;
        const float dF = coef * rres;
        const float gv = okc[ct] ? dF * e * 0.5f / sd : 0.f;
        if (okc[ct] && kq == 0) {
          const long long o = (long long)l * C + cw + ct * 16 + j;
          a.g[o] = gv;
          a.dmeanT[o] = dF;
          if (a.FT != nullptr) a.FT[o] = Fd;
          const float z = rres * inv;
          z2l += z * z;
        }
        // g_l W_l into the second set (AGPRs, as panel_elbo_kernel; the unit is built with -amdgpu-mfma-vgpr-form)
#pragma unroll
        for (int rt = 0; rt < MB; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float t;
            asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(ab[rt][ct][r]));
            t = fmaf(gv, acc[rt][ct][r], t);
            asm("v_accvgpr_write_b32 %0, %1" : "=a"(ab[rt][ct][r]) : "v"(t));
          }
      }
      z2 += (double)z2l;
    }
    {
      const bool pl = (l_lo == 0) && (l_hi == L - 1);
      const int which = (tile == ord.tile0) ? 0 : 1;
      float* dst = pl ? a.abar : a.slab + ((long long)blockIdx.x * 2 + which) * MP * WGCOLS;
      const long long rs = pl ? C : (long long)WGCOLS;
      const int mlim = pl ? M : MP;
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) {
        const long long c = cw + ct * 16 + j;
        const long long col = pl ? c : (long long)(w * (16 * NCT) + ct * 16 + j);
        const bool ok = pl ? (c < C) : true;
#pragma unroll
        for (int rt = 0; rt < MB; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = rt * 16 + kq * 4 + r;
            float t;
            asm("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(ab[rt][ct][r]));
            if (ok && row < mlim) dst[(long long)row * rs + col] = 2.f * t;
          }
      }
    }
  }
  GPSA_DMA_DRAIN();
  z2 = block_sum(z2, red);
  if (tid == 0) a.part[blockIdx.x] = z2;
#undef GPSA_X3_STAGE
}

GPSA_ELBO_X3_SHAPES(GPSA_ELBO_X3_DEFINE)

// ------------------------------------------------------------------------------------------------
// gram_x3_kernel: dOmega_l = sum_c g[l,c] alpha_c alpha_c^T (and the d-delta option) in three bf16 pieces.
// alpha is split ONCE per call into a three-plane image (split_image_kernel): [KBc][MB][3][64 lanes][8] bf16, piece
// (kb, rt, plane) the fragment of row tile rt over columns 32 kb .. + 31, lane i + 16 kq holding columns 8 kq .. + 7 of
// row 16 rt + i (zero past M and C).  The column fragments (B) are the image's pieces as they are; the g-scaled row
// fragment (A) is rebuilt from the pieces ((a1 + a2) + a3 = alpha exactly), scaled by g and split again, once per row
// and K block - as the fp32 kernel scales its row fragment once per row and K block.  Grid (L, nsplit): workgroup
// (l, s) sweeps its share of the 32-column chunks, staged by LDS-DMA into two slots (one MB x 3 KiB chunk in flight while
// the other is multiplied); the lower-triangle tiles are dealt to the waves by whole rows (GramPlan).  Partials
// [L][nsplit][MP][MP] are added in a fixed order by gram_reduce_kernel: no atomics, bitwise repeatable.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) split_image_kernel(const float* __restrict__ X, int M, int MB, long long C, long long KBc,
                                                          unsigned short* __restrict__ dst) {
  const long long idx = blockIdx.x * 256LL + threadIdx.x;  // one thread per (kb, rt, lane)
  if (idx >= KBc * MB * 64) return;
  const long long kb = idx / (MB * 64);
  const int rt = (int)(idx / 64 % MB), lane = (int)(idx % 64);
  const int row = rt * 16 + (lane & 15);
  const long long c0 = kb * 32 + (lane >> 4) * 8;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (row < M && c0 + e < C) ? X[(long long)row * C + c0 + e] : 0.f;
  x3_bf16x8 p[3];
  x3_split(v, p);
  x3_bf16x8* out = reinterpret_cast<x3_bf16x8*>(dst) + (kb * MB + rt) * 3 * 64 + lane;
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q * 64] = p[q];
}

constexpr int GX_G = 4;  // tiles whose MFMAs are interleaved (an accumulator is touched every fourth MFMA)

template <int MB, int W>
__device__ __forceinline__ void gram_x3_wave(const unsigned short* __restrict__ img, const float* __restrict__ g,
                                             const float* __restrict__ dmean, int M, long long C, int L, int nsplit,
                                             float* __restrict__ part, unsigned short* lds, int slot_elems) {
  constexpr GramPlan<MB> P{};
  constexpr int N = P.cnt[W];
  constexpr int MP = MB * 16;
  constexpr int NPIECE = MB * 3, NPW = (NPIECE + 3) / 4, CHUNK = NPIECE * 512;
  constexpr bool OWNS_LAST = [] {
    constexpr GramPlan<MB> Q{};
    for (int s = 0; s < Q.cnt[W]; ++s)
      if (Q.rr[W][s] == MB - 1) return true;
    return false;
  }();
  const int lane = threadIdx.x & 63, j = lane & 15, kq = lane >> 4;
  const int l = blockIdx.x, sp = blockIdx.y;
  const long long KBc = (C + 31) / 32;
  const long long ch0 = (long long)sp * KBc / nsplit, ch1 = (long long)(sp + 1) * KBc / nsplit;
  const int drow = dmean != nullptr ? M - 16 * (MB - 1) : -1;
  const bool dsel = OWNS_LAST && drow >= 0 && j == drow;

  f32x4 acc[N > 0 ? N : 1];
#pragma unroll
  for (int s = 0; s < N; ++s) acc[s] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // this lane's 8 values of g (and of dmean) for chunk ch: columns 32 ch + 8 kq .. + 7
  auto load8 = [&](const float* row, long long ch, float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long long c = ch * 32 + kq * 8 + e;
      v[e] = c < C ? row[c < C ? c : 0] : 0.f;
    }
  };
  auto stage = [&](long long ch, int buf) {
    const unsigned short* src0 = img + ch * CHUNK + lane * 8;
#pragma unroll
    for (int pc = 0; pc < NPW; ++pc) {
      const int piece = pc * 4 + W;
      glds16(reinterpret_cast<const float*>(src0 + (piece < NPIECE ? piece : NPIECE - 1) * 512),
             __builtin_amdgcn_readfirstlane(lds_addr(lds + buf * slot_elems + piece * 512)));
    }
  };
  const float* grow = g + (long long)l * C;
  const float* drow_p = dmean != nullptr ? dmean + (long long)l * C : nullptr;
  float gn[8], dn[8];
  if (ch1 > ch0) {
    load8(grow, ch0, gn);
    if (OWNS_LAST && drow_p != nullptr) load8(drow_p, ch0, dn);
    stage(ch0, 0);
  }
  GPSA_DMA_DRAIN();
  __syncthreads();
  int buf = 0;
  for (long long ch = ch0; ch < ch1; ++ch) {
    float gk[8], dk[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gk[e] = gn[e];
      dk[e] = (OWNS_LAST && drow_p != nullptr) ? dn[e] : 0.f;
    }
    // the next chunk's g (compiler-visible loads first, then the DMA: waiting for the loads never waits for the stage)
    if (ch + 1 < ch1) {
      load8(grow, ch + 1, gn);
      if (OWNS_LAST && drow_p != nullptr) load8(drow_p, ch + 1, dn);
      stage(ch + 1, buf ^ 1);
    }
    const unsigned short* base = lds + buf * slot_elems + lane * 8;
    x3_bf16x8 arow[3];
#pragma unroll
    for (int g0 = 0; g0 < N; g0 += GX_G) {
      x3_bf16x8 a[GX_G][3], b[GX_G][3];
#pragma unroll
      for (int u = 0; u < GX_G; ++u) {
        const int s = g0 + u < N ? g0 + u : N - 1;
        const int rr = P.rr[W][s], cc = P.cc[W][s];
        if (g0 + u < N && (s == 0 || P.rr[W][s] != P.rr[W][s > 0 ? s - 1 : 0])) {
          // new row: its g-scaled fragment, rebuilt, scaled and split
          x3_bf16x8 r3[3];
#pragma unroll
          for (int q = 0; q < 3; ++q) r3[q] = *reinterpret_cast<const x3_bf16x8*>(base + (rr * 3 + q) * 512);
          float v[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = ((float)r3[0][e] + (float)r3[1][e]) + (float)r3[2][e];
            v[e] = x * gk[e];
            if (OWNS_LAST && rr == MB - 1) v[e] = dsel ? dk[e] : v[e];
          }
          x3_split(v, arow);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          a[u][q] = arow[q];
          b[u][q] = *reinterpret_cast<const x3_bf16x8*>(base + (cc * 3 + q) * 512);
        }
      }
      // smallest products first, the tiles of the group interleaved
#define GPSA_GX_MMA(IA, IB)                                                                      \
  _Pragma("unroll") for (int u = 0; u < GX_G; ++u) if (g0 + u < N)                               \
    acc[g0 + u < N ? g0 + u : 0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(                      \
        a[u][IA], b[u][IB], acc[g0 + u < N ? g0 + u : 0], 0, 0, 0);
      GPSA_GX_MMA(2, 0)
      GPSA_GX_MMA(1, 1)
      GPSA_GX_MMA(0, 2)
      GPSA_GX_MMA(1, 0)
      GPSA_GX_MMA(0, 1)
      GPSA_GX_MMA(0, 0)
#undef GPSA_GX_MMA
      __builtin_amdgcn_sched_barrier(0);
    }
    GPSA_DMA_DRAIN();  // the next chunk has landed
    __syncthreads();   // and every wave is done with this slot
    buf ^= 1;
  }
  float* Pp = part + ((long long)l * nsplit + sp) * MP * MP;
#pragma unroll
  for (int s = 0; s < N; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) Pp[(long long)(P.rr[W][s] * 16 + kq * 4 + r) * MP + P.cc[W][s] * 16 + j] = acc[s][r];
}

template <int MB>
__global__ void __launch_bounds__(256, 1) gram_x3_kernel(const unsigned short* __restrict__ img, const float* __restrict__ g,
                                                         const float* __restrict__ dmean, int M, long long C, int L,
                                                         int nsplit, float* __restrict__ part) {
  constexpr int NPW = (MB * 3 + 3) / 4, SLOT = NPW * 4 * 512;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * SLOT];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  switch (w) {
    case 0: gram_x3_wave<MB, 0>(img, g, dmean, M, C, L, nsplit, part, lds, SLOT); break;
    case 1: gram_x3_wave<MB, 1>(img, g, dmean, M, C, L, nsplit, part, lds, SLOT); break;
    case 2: gram_x3_wave<MB, 2>(img, g, dmean, M, C, L, nsplit, part, lds, SLOT); break;
    default: gram_x3_wave<MB, 3>(img, g, dmean, M, C, L, nsplit, part, lds, SLOT); break;
  }
}
#define GPSA_GRAM_X3_DEFINE(MB)                                                                                   \
  template __global__ void gram_x3_kernel<MB>(const unsigned short* __restrict__, const float* __restrict__,       \
                                              const float* __restrict__, int, long long, int, int, float* __restrict__);
GPSA_GRAM_X3_SHAPES(GPSA_GRAM_X3_DEFINE)

}  // namespace gpsa
