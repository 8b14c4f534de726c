// The body that lmc_mfma_kernel, lmc_mfma_skip_kernel and lmc_mfma_pois_kernel (lmc.hip) share.  It is a FRAGMENT: each
// kernel includes it between its braces, after ``constexpr bool SKIP = ...`` and the likelihood selector ``constexpr int
// LIK = GPSA_LIK_...``, with the template parameters NLT, NPT and the kernel's arguments (F, W, Y, noise_u, S, N, L, P,
// zpart, nparts, dF, dWpart; the Gaussian kernels define log_offset as a constexpr nullptr, the Poisson kernel has it as
// an argument, noise_u as a constexpr nullptr and SKIP as a run-time flag) in scope.  Textual inclusion, not a device
// function: the default kernel's code then is what it was before the skip variant existed, instruction for instruction
// (an inlined function taking the arguments moved its register allocation: 193/193/223 registers became 200/196/230),
// and the two kernels differ by the one compare in the residual's select.
// LIK == GPSA_LIK_POISSON: fo[r] is the log rate, eta = fo + log_offset[row] (a per-row load next to Yr),
// dfo = (exp(eta) - y) / S with the exact expf, the summed term y eta - exp(eta); the dW and dF chains are unchanged.
// LIK == GPSA_LIK_NEGBIN (lmc_mfma_nb_kernel; the other kernels define log_disp and upart as constexpr nullptrs): fo[r] is
// the log mean, a = fo + log_offset[row] - rho_p with rho_p = log_disp[p] loaded once per chunk of outputs (the thread's
// columns), dfo = ((y + r) sigma(a) - y) / S, the summed term t = y a - (y + r) softplus(a), and u = -r softplus(a) +
// (y + r) sigma(a) - y summed per output in fp64 registers: a wave owns its outputs of the chunk, so the four row groups
// of a lane column meet by two lane exchanges and upart[workgroup][p] is written once per chunk, next to dWpart.
  constexpr int LT = 16 * NLT, KB = 4 * NLT, PC = 64 * NPT, WS = PC + 4, FS = LT + 1;
  extern __shared__ __attribute__((aligned(16))) float lm_smem[];
  float* sW = lm_smem;                   // [LT][WS]   W[l][p0 + pp], zero padded
  float* sF = sW + LT * WS;              // [16][FS]   the tile's draws F[c][l], zero padded
  float* sT = sF + 16 * FS;              // [4][16][17] a wave's dfo tile, for the transposition
  float* sR = sT + 4 * 16 * 17;          // [4][LT][17] the waves' partial dF^T tiles
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const double sN = LIK != GPSA_LIK_GAUSSIAN ? 1.0 : exp((double)noise_u[0]) + 1e-5;  // "variance" used as std
  const float inv = (float)(1.0 / sN);
  const float coef = LIK != GPSA_LIK_GAUSSIAN ? (float)(1.0 / (double)S) : (float)(-1.0 / (sN * sN * (double)S));
  const long long ntiles = (N + 15) / 16;
  double z2 = 0.0;
  float* sTw = sT + w * 16 * 17;

  for (int p0 = 0; p0 < P; p0 += PC) {
    __syncthreads();  // (the previous chunk's readers of sW are done)
    for (int e = tid; e < LT * PC; e += 256) {
      const int l = e / PC, pp = e - l * PC;
      sW[l * WS + pp] = (l < L && p0 + pp < P) ? W[(long long)l * P + p0 + pp] : 0.f;
    }
    __syncthreads();
    const int pw = w * 16 * NPT;  // this wave's first output of the chunk
    float Wf[NPT][KB];            // B fragments of fobs = F W: W[4 ks + kq][p]
#pragma unroll
    for (int i = 0; i < NPT; ++i)
#pragma unroll
      for (int ks = 0; ks < KB; ++ks) Wf[i][ks] = sW[(4 * ks + kq) * WS + pw + 16 * i + li];
    lm_f32x4 dWacc[NPT][NLT];
#pragma unroll
    for (int i = 0; i < NPT; ++i)
#pragma unroll
      for (int lt = 0; lt < NLT; ++lt) dWacc[i][lt] = (lm_f32x4){0.f, 0.f, 0.f, 0.f};
    bool pok[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) pok[i] = p0 + pw + 16 * i + li < P;
    float rh[NPT], rsz[NPT];  // (NB) rho and r = exp(rho) of this thread's outputs
    double uacc[NPT];         // (NB) their sums of u over this workgroup's tiles
    if constexpr (LIK == GPSA_LIK_NEGBIN) {
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        rh[i] = log_disp[pok[i] ? p0 + pw + 16 * i + li : P - 1];
        rsz[i] = expf(rh[i]);
        uacc[i] = 0.0;
      }
    }

    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
      const long long n0 = t * 16;
      // the tile's observations in the accumulator layout: column p = lane & 15 of output tile i, rows 4 kq + r
      float Yr[NPT][4];
      float Or[4];  // (Poisson) the rows' log offsets
      bool rok[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        rok[r] = n0 + 4 * kq + r < N;
        if constexpr (LIK != GPSA_LIK_GAUSSIAN)
          Or[r] = log_offset != nullptr ? log_offset[rok[r] ? n0 + 4 * kq + r : N - 1] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < NPT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long row = rok[r] ? n0 + 4 * kq + r : N - 1;
          const int p = pok[i] ? p0 + pw + 16 * i + li : P - 1;
          Yr[i][r] = Y[row * P + p];
        }
      for (int s = 0; s < S; ++s) {
        const long long c0 = (long long)s * N + n0;
        for (int e = tid; e < 16 * LT; e += 256) {
          const int cc = e / LT, l = e - cc * LT;
          sF[cc * FS + l] = (n0 + cc < N && l < L) ? F[(c0 + cc) * L + l] : 0.f;
        }
        __syncthreads();  // (A) the tile's draws are staged
        float aF[KB], aT[4][NLT];
#pragma unroll
        for (int ks = 0; ks < KB; ++ks) aF[ks] = sF[li * FS + 4 * ks + kq];        // A of fobs: F[c = li][l = 4 ks + kq]
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int lt = 0; lt < NLT; ++lt) aT[r][lt] = sF[(4 * kq + r) * FS + 16 * lt + li];  // A of dW: F[c = 4 kq + r][l]
        lm_f32x4 accF[NLT];
#pragma unroll
        for (int lt = 0; lt < NLT; ++lt) accF[lt] = (lm_f32x4){0.f, 0.f, 0.f, 0.f};
        float z2l = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
          lm_f32x4 fo = (lm_f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KB; ++ks) fo = __builtin_amdgcn_mfma_f32_16x16x4f32(aF[ks], Wf[i][ks], fo, 0, 0, 0);
          float dfo[4];
          float ul = 0.f;  // (NB) this output's u over the four rows
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (LIK == GPSA_LIK_NEGBIN) {
              const float a = fo[r] + Or[r] - rh[i];
              const float e = expf(-fabsf(a));                    // in (0, 1]: nothing overflows
              const float sp = fmaxf(a, 0.f) + log1pf(e);         // softplus(a)
              const float sg = (a >= 0.f ? 1.f : e) / (1.f + e);  // sigma(a)
              const float y = Yr[i][r], yr = y + rsz[i];
              const bool obs = rok[r] && pok[i] && (!SKIP || y == y);
              const float d = fmaf(yr, sg, -y);
              z2l += obs ? fmaf(y, a, -yr * sp) : 0.f;
              ul += obs ? fmaf(-rsz[i], sp, d) : 0.f;
              dfo[r] = obs ? coef * d : 0.f;
            } else if constexpr (LIK == GPSA_LIK_POISSON) {
              const float eta = fo[r] + Or[r];
              const float ex = expf(eta);
              const bool obs = rok[r] && pok[i] && (!SKIP || Yr[i][r] == Yr[i][r]);
              z2l += obs ? fmaf(Yr[i][r], eta, -ex) : 0.f;
              dfo[r] = obs ? coef * (ex - Yr[i][r]) : 0.f;
            } else {
              const float rr = (rok[r] && pok[i] && (!SKIP || Yr[i][r] == Yr[i][r])) ? Yr[i][r] - fo[r] : 0.f;
              const float z = rr * inv;
              z2l = fmaf(z, z, z2l);
              dfo[r] = coef * rr;
            }
          }
          if constexpr (LIK == GPSA_LIK_NEGBIN) uacc[i] += (double)ul;
          // dW[l, p] += sum_c F[c, l] dfo[c, p]: K step r contracts the spots 4 kq + r
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int lt = 0; lt < NLT; ++lt)
              dWacc[i][lt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aT[r][lt], dfo[r], dWacc[i][lt], 0, 0, 0);
          // dF^T[l, c] += sum_p W[l, p] dfo[c, p]: the dfo tile transposed through this wave's LDS tile (a wave's LDS
          // operations execute in order: no barrier between its writes and its reads)
#pragma unroll
          for (int r = 0; r < 4; ++r) sTw[(4 * kq + r) * 17 + li] = dfo[r];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            const float bT = sTw[li * 17 + 4 * ks + kq];  // B[k = p = 4 ks + kq][n = c = li]
#pragma unroll
            for (int lt = 0; lt < NLT; ++lt) {
              const float aW = sW[(16 * lt + li) * WS + pw + 16 * i + 4 * ks + kq];  // A[m = l][k = p]
              accF[lt] = __builtin_amdgcn_mfma_f32_16x16x4f32(aW, bT, accF[lt], 0, 0, 0);
            }
          }
        }
        z2 += (double)z2l;
        // the four waves' shares of dF^T[l = 16 lt + 4 kq + r][c = li] meet in LDS
        float* sRw = sR + w * LT * 17;
#pragma unroll
        for (int lt = 0; lt < NLT; ++lt)
#pragma unroll
          for (int r = 0; r < 4; ++r) sRw[(16 * lt + 4 * kq + r) * 17 + li] = accF[lt][r];
        __syncthreads();  // (B) every wave is done with sF and has left its share
        for (int e = tid; e < 16 * LT; e += 256) {
          const int l = e >> 4, cc = e & 15;
          if (l < L && n0 + cc < N) {
            const float sum = (sR[l * 17 + cc] + sR[(LT + l) * 17 + cc]) + (sR[(2 * LT + l) * 17 + cc] + sR[(3 * LT + l) * 17 + cc]);
            const long long o = (c0 + cc) * L + l;
            dF[o] = p0 == 0 ? sum : dF[o] + sum;  // (this workgroup owns the tile in every chunk of p)
          }
        }
        // (the next sample's staging of sF may start: nobody reads sF before its barrier (A); sR is rewritten only
        //  after that barrier, when these sums are done)
      }
    }
    // this workgroup's share of dW for the chunk: rows l = 16 lt + 4 kq + r, column p = lane & 15 of tile i
#pragma unroll
    for (int i = 0; i < NPT; ++i)
#pragma unroll
      for (int lt = 0; lt < NLT; ++lt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = 16 * lt + 4 * kq + r, p = p0 + pw + 16 * i + li;
          if (l < L && p < P) dWpart[((long long)blockIdx.x * L + l) * P + p] = dWacc[i][lt][r];
        }
    if constexpr (LIK == GPSA_LIK_NEGBIN) {
      // this workgroup's sums of u for the chunk: the row groups kq of a column in the fixed order (0 + 1) + (2 + 3)
#pragma unroll
      for (int i = 0; i < NPT; ++i) {
        double v = uacc[i];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        const int p = p0 + pw + 16 * i + li;
        if (kq == 0 && p < P) upart[(long long)blockIdx.x * P + p] = v;
      }
    }
  }
  z2 = block_sum(z2, red);
  if (tid == 0) zpart[blockIdx.x] = z2;
  if (blockIdx.x == 0)
    for (int i = (int)gridDim.x + tid; i < nparts; i += 256) zpart[i] = 0.0;
