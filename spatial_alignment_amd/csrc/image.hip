// Histology images on the device: the pixel modality out of an image (select) and an image read at arbitrary pixel
// coordinates (sample).  img is [H, W, C] row-major, C in 1..4, uint8 (a value is (float)u / 255.0f, one fp32 division)
// or fp32 (taken as is).  As in counts.hip and neighbors.hip: no atomics, every sum in a fixed order, one writer per
// output element, the same bits on a repeated call, every refusal before the first launch, and nothing of H W elements
// is allocated.
//
// select.  `bin` = b reduces the image to H' = H div b, W' = W div b output pixels; output pixel (r, c) is the mean of
// its full b x b block per channel (an fp64 sum in row-major order within the block, divided by b^2 in fp64, rounded to
// fp32 once; partial blocks at the right and bottom edges are dropped) and lies at x = c b + (b - 1) / 2,
// y = r b + (b - 1) / 2.  image_classify gives its class:
//   background: every channel has rintf(v * 10.0f) == rintf(bg * 10.0f)   (np.round(v, 1) == bg in fp32; a NaN channel is
//               never background; has_bg = 0: no pixel is)
//   outside:    not background, and not xmin < x < xmax && ymin < y < ymax (strict, fp64; has_bbox = 0: no pixel is)
//   kept:       the rest.
// The output pixels are cut, in row-major order, into tiles of IMG_SELECT_TILE; a workgroup of IMG_SELECT_THREADS takes a
// tile in IMG_SELECT_TILE / IMG_SELECT_THREADS rounds of consecutive pixels, so a wave's loads of a bin = 1 image are
// contiguous.
//   * image_count_kernel: per tile the three class counts (wave ballots and popcounts, the four waves' totals meet in
//     LDS in wave order) -> cnt [T, 3] int32;
//   * image_scan_kernel, ONE workgroup: thread t sums the counts of the tiles [t ch, (t + 1) ch) in order, one thread per
//     class scans the IMG_SELECT_THREADS sums in order, every thread writes its tiles' exclusive kept offsets -> off [T]
//     int64, and the totals (kept, background, outside) -> tot [3] int64 at the head of the workspace;
//   * image_write_kernel recomputes the class; a kept pixel's row is off[tile] + the kept pixels of the earlier rounds +
//     the earlier waves' kept pixels of this round (LDS) + the popcount of the ballot below its lane: a stable compaction,
//     coords [n, 2] fp32 = (x, y), pixels [n, C] fp32 in the row-major order of the output pixels.  A row at or beyond
//     `capacity` is never stored.
// Workspace (gpsa_image_select_workspace): tot [4] int64, off [T] int64, cnt [T, 3] int32.
//
// sample.  One thread per row of xy [n, 2] fp64 (x the column, y the row): valid when 0 <= x <= W - 1 && 0 <= y <= H - 1
// (NaN and +-inf fail); an invalid row reads nothing and is `fill`.  order 1 is bilinear in fp64 without contraction,
// rounded to fp32 once, on the cell x0 = min(floor(x), W - 2) (0 when W = 1), so x = W - 1 never reads column W; order 0
// is the pixel at floor(x + 0.5), clamped into the image.
#include <math.h>

#include "common.hpp"

namespace gpsa {

constexpr int IMG_SELECT_THREADS = 256;  // a workgroup: four waves
constexpr int IMG_SELECT_TILE = 2048;    // output pixels of a tile: 8 rounds of IMG_SELECT_THREADS
constexpr int IMG_WAVES = IMG_SELECT_THREADS / WAVE;
constexpr int IMG_MAX_C = 4, IMG_MAX_BIN = 64;
constexpr int IMG_SAMPLE_THREADS = 256;

enum { IMG_KEPT = 0, IMG_BACKGROUND = 1, IMG_OUTSIDE = 2, IMG_NONE = 3 };

struct ImageSelect {  // what the three select kernels share
  long long H, W, Ho, Wo, n_out;
  int C, bin, has_bg, has_bbox;
  float bg;
  double xmin, xmax, ymin, ymax;
};

struct ImageWorkspace {
  long long *tot = nullptr, *off = nullptr;
  int* cnt = nullptr;
  long long T, bytes;
  ImageWorkspace(void* ws, long long H, long long W, long long bin) {
    T = cdiv((H / bin) * (W / bin), (long long)IMG_SELECT_TILE);
    bytes = 8 * (4 + T) + 4 * ((3 * T + 1) / 2 * 2);
    if (ws == nullptr) return;  // the size alone
    tot = (long long*)ws, off = tot + 4, cnt = (int*)(off + T);
  }
};

__device__ __forceinline__ float image_value(unsigned char u) { return (float)u / 255.0f; }
__device__ __forceinline__ float image_value(float f) { return f; }

// the class of output pixel p < n_out, its channels in v and its coordinate in (x, y)
template <typename T>
__device__ __forceinline__ int image_classify(const T* __restrict__ img, const ImageSelect& s, long long p, float* v,
                                              double& x, double& y) {
  const long long r = p / s.Wo, c = p - r * s.Wo;
  const int b = s.bin;
  if (b == 1) {
    const T* px = img + (r * s.W + c) * s.C;
    for (int ch = 0; ch < s.C; ++ch) v[ch] = image_value(px[ch]);
  } else {
    double acc[IMG_MAX_C] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < b; ++i) {
      const T* row = img + ((r * b + i) * s.W + c * b) * s.C;
      for (int j = 0; j < b; ++j)
        for (int ch = 0; ch < s.C; ++ch) acc[ch] += (double)image_value(row[j * s.C + ch]);
    }
    const double area = (double)(b * b);
    for (int ch = 0; ch < s.C; ++ch) v[ch] = (float)(acc[ch] / area);
  }
  const double half = 0.5 * (double)(b - 1);
  x = (double)(c * b) + half, y = (double)(r * b) + half;
  if (s.has_bg) {
    const float q = rintf(s.bg * 10.0f);
    bool all = true;
    for (int ch = 0; ch < s.C; ++ch) all = all && (rintf(v[ch] * 10.0f) == q);
    if (all) return IMG_BACKGROUND;
  }
  if (s.has_bbox && !(s.xmin < x && x < s.xmax && s.ymin < y && y < s.ymax)) return IMG_OUTSIDE;
  return IMG_KEPT;
}

__device__ __forceinline__ int ballot_count(bool pred) { return (int)__popcll(__builtin_amdgcn_ballot_w64(pred)); }

template <typename T>
__global__ void __launch_bounds__(IMG_SELECT_THREADS)
image_count_kernel(const T* __restrict__ img, ImageSelect s, int* __restrict__ cnt) {
  __shared__ int wc[IMG_WAVES][3];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * IMG_SELECT_TILE;
  int n_kept = 0, n_bg = 0, n_out = 0;  // wave-uniform
  for (int q = 0; q < IMG_SELECT_TILE; q += IMG_SELECT_THREADS) {
    const long long p = base + q + threadIdx.x;
    float v[IMG_MAX_C];
    double x, y;
    const int cls = p < s.n_out ? image_classify(img, s, p, v, x, y) : IMG_NONE;
    n_kept += ballot_count(cls == IMG_KEPT);
    n_bg += ballot_count(cls == IMG_BACKGROUND);
    n_out += ballot_count(cls == IMG_OUTSIDE);
  }
  if (lane == 0) wc[w][0] = n_kept, wc[w][1] = n_bg, wc[w][2] = n_out;
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
    for (int k = 0; k < IMG_WAVES; ++k) t += wc[k][threadIdx.x];
    cnt[3 * (long long)blockIdx.x + threadIdx.x] = t;
  }
}

// one workgroup; see the head of the file
__global__ void __launch_bounds__(IMG_SELECT_THREADS)
image_scan_kernel(const int* __restrict__ cnt, long long T, long long* __restrict__ off, long long* __restrict__ tot) {
  __shared__ long long part[3][IMG_SELECT_THREADS];
  const long long ch = (T + IMG_SELECT_THREADS - 1) / IMG_SELECT_THREADS;
  const long long t0 = min(T, (long long)threadIdx.x * ch), t1 = min(T, t0 + ch);
  long long mine[3] = {0, 0, 0};
  for (long long t = t0; t < t1; ++t)
    for (int k = 0; k < 3; ++k) mine[k] += cnt[3 * t + k];
  for (int k = 0; k < 3; ++k) part[k][threadIdx.x] = mine[k];
  __syncthreads();
  if (threadIdx.x < 3) {  // a class each: the threads' sums in order; the kept ones become exclusive offsets
    long long run = 0;
    for (int k = 0; k < IMG_SELECT_THREADS; ++k) {
      const long long here = part[threadIdx.x][k];
      part[threadIdx.x][k] = run, run += here;
    }
    tot[threadIdx.x] = run;
  }
  __syncthreads();
  long long run = part[IMG_KEPT][threadIdx.x];
  for (long long t = t0; t < t1; ++t) off[t] = run, run += cnt[3 * t];
}

template <typename T>
__global__ void __launch_bounds__(IMG_SELECT_THREADS)
image_write_kernel(const T* __restrict__ img, ImageSelect s, const long long* __restrict__ off, long long capacity,
                   float* __restrict__ coords, float* __restrict__ pixels) {
  __shared__ int wt[2][IMG_WAVES];  // the waves' kept counts of a round; two copies: one barrier per round
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * IMG_SELECT_TILE;
  long long row0 = off[blockIdx.x];  // the first row of this round
  int buf = 0;
  for (int q = 0; q < IMG_SELECT_TILE; q += IMG_SELECT_THREADS, buf ^= 1) {
    const long long p = base + q + threadIdx.x;
    float v[IMG_MAX_C];
    double x = 0.0, y = 0.0;
    const bool kept = p < s.n_out && image_classify(img, s, p, v, x, y) == IMG_KEPT;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(kept);
    if (lane == 0) wt[buf][w] = (int)__popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < IMG_WAVES; ++k) {
      const int here = wt[buf][k];
      before += k < w ? here : 0, total += here;
    }
    const long long row = row0 + before + (long long)__popcll(mask & ((1ULL << lane) - 1ULL));
    if (kept && row >= 0 && row < capacity) {
      coords[2 * row] = (float)x, coords[2 * row + 1] = (float)y;
      for (int ch = 0; ch < s.C; ++ch) pixels[row * s.C + ch] = v[ch];
    }
    row0 += total;
  }
}

template <typename T>
__global__ void __launch_bounds__(IMG_SAMPLE_THREADS)
image_sample_kernel(const T* __restrict__ img, long long H, long long W, int C, const double* __restrict__ xy,
                    long long n, int order, float fill, float* __restrict__ out, unsigned char* __restrict__ valid) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * IMG_SAMPLE_THREADS + threadIdx.x;
  if (i >= n) return;
  const double x = xy[2 * i], y = xy[2 * i + 1];
  const bool ok = x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1);
  valid[i] = ok ? 1 : 0;
  if (!ok) {
    for (int ch = 0; ch < C; ++ch) out[i * C + ch] = fill;
    return;
  }
  if (order == 0) {
    const long long xi = min(max((long long)floor(x + 0.5), 0LL), W - 1);
    const long long yi = min(max((long long)floor(y + 0.5), 0LL), H - 1);
    const T* px = img + (yi * W + xi) * C;
    for (int ch = 0; ch < C; ++ch) out[i * C + ch] = image_value(px[ch]);
    return;
  }
  const long long x0 = W > 1 ? min((long long)floor(x), W - 2) : 0, x1 = min(x0 + 1, W - 1);
  const long long y0 = H > 1 ? min((long long)floor(y), H - 2) : 0, y1 = min(y0 + 1, H - 1);
  const double fx = x - (double)x0, fy = y - (double)y0;
  const T *p00 = img + (y0 * W + x0) * C, *p01 = img + (y0 * W + x1) * C;
  const T *p10 = img + (y1 * W + x0) * C, *p11 = img + (y1 * W + x1) * C;
  for (int ch = 0; ch < C; ++ch) {
    const double top = (double)image_value(p00[ch]) * (1.0 - fx) + (double)image_value(p01[ch]) * fx;
    const double bot = (double)image_value(p10[ch]) * (1.0 - fx) + (double)image_value(p11[ch]) * fx;
    out[i * C + ch] = (float)(top * (1.0 - fy) + bot * fy);
  }
}

// what every select entry asks of its sizes: 0 or GPSA_EINVAL
static int image_shape_check(long long H, long long W, int C, int bin) {
  if (H < 1 || W < 1 || C < 1 || C > IMG_MAX_C || bin < 1 || bin > IMG_MAX_BIN || bin > H || bin > W) return GPSA_EINVAL;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || (H / bin) * (W / bin) >= 0x80000000LL) return GPSA_EINVAL;
  return 0;
}

static ImageSelect image_select_args(long long H, long long W, int C, int bin, int has_bg, float bg, int has_bbox,
                                     const double* bbox) {
  ImageSelect s;
  s.H = H, s.W = W, s.Ho = H / bin, s.Wo = W / bin, s.n_out = s.Ho * s.Wo;
  s.C = C, s.bin = bin, s.has_bg = has_bg ? 1 : 0, s.has_bbox = has_bbox ? 1 : 0, s.bg = bg;
  s.xmin = has_bbox ? bbox[0] : 0.0, s.xmax = has_bbox ? bbox[1] : 0.0;
  s.ymin = has_bbox ? bbox[2] : 0.0, s.ymax = has_bbox ? bbox[3] : 0.0;
  return s;
}

static int image_select_check(const void* img, long long H, long long W, int C, int bin, int has_bbox,
                              const double* bbox, const void* workspace, long long workspace_bytes) {
  if (int rc = image_shape_check(H, W, C, bin)) return rc;
  if (img == nullptr) return GPSA_EINVAL;
  if (has_bbox) {
    if (bbox == nullptr) return GPSA_EINVAL;
    for (int k = 0; k < 4; ++k)
      if (bbox[k] != bbox[k]) return GPSA_EINVAL;
  }
  if (workspace == nullptr || workspace_bytes < ImageWorkspace(nullptr, H, W, bin).bytes) return GPSA_EWORKSPACE;
  return 0;
}

template <typename T>
static int image_select_count(const T* img, long long H, long long W, int C, int bin, int has_bg, float bg, int has_bbox,
                              const double* bbox, void* workspace, long long workspace_bytes, hipStream_t st) {
  if (int rc = image_select_check(img, H, W, C, bin, has_bbox, bbox, workspace, workspace_bytes)) return rc;
  const ImageWorkspace ws(workspace, H, W, bin);
  const ImageSelect s = image_select_args(H, W, C, bin, has_bg, bg, has_bbox, bbox);
  image_count_kernel<T><<<(unsigned)ws.T, IMG_SELECT_THREADS, 0, st>>>(img, s, ws.cnt);
  GPSA_LAUNCH_CHECK();
  image_scan_kernel<<<1, IMG_SELECT_THREADS, 0, st>>>(ws.cnt, ws.T, ws.off, ws.tot);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int image_select_write(const T* img, long long H, long long W, int C, int bin, int has_bg, float bg, int has_bbox,
                              const double* bbox, void* workspace, long long workspace_bytes, float* coords,
                              float* pixels, long long capacity, hipStream_t st) {
  if (int rc = image_select_check(img, H, W, C, bin, has_bbox, bbox, workspace, workspace_bytes)) return rc;
  if (coords == nullptr || pixels == nullptr || capacity < 1) return GPSA_EINVAL;
  const ImageWorkspace ws(workspace, H, W, bin);
  // the kept total of the count pass, from the workspace the caller passes back: one small read, as the caller's own
  long long kept = -1;
  hipError_t e = hipMemcpyAsync(&kept, ws.tot, sizeof(kept), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return (int)e;
  if (kept < 0 || kept > capacity) return GPSA_EINVAL;
  if (kept == 0) return 0;
  const ImageSelect s = image_select_args(H, W, C, bin, has_bg, bg, has_bbox, bbox);
  image_write_kernel<T><<<(unsigned)ws.T, IMG_SELECT_THREADS, 0, st>>>(img, s, ws.off, kept, coords, pixels);
  GPSA_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int image_sample(const T* img, long long H, long long W, int C, const double* xy, long long n, int order,
                        float fill, float* out, unsigned char* valid, hipStream_t st) {
  if (img == nullptr || xy == nullptr || out == nullptr || valid == nullptr) return GPSA_EINVAL;
  if (H < 1 || W < 1 || H > 0x7fffffffLL || W > 0x7fffffffLL || C < 1 || C > IMG_MAX_C) return GPSA_EINVAL;
  if (n < 1 || n > 0x7fffffffLL || (order != 0 && order != 1)) return GPSA_EINVAL;
  image_sample_kernel<T><<<(unsigned)cdiv(n, (long long)IMG_SAMPLE_THREADS), IMG_SAMPLE_THREADS, 0, st>>>(
      img, H, W, C, xy, n, order, fill, out, valid);
  GPSA_LAUNCH_CHECK();
  return 0;
}

}  // namespace gpsa

extern "C" {

long long gpsa_image_select_workspace(long long H, long long W, int bin) {
  if (gpsa::image_shape_check(H, W, 1, bin)) return 0;
  return gpsa::ImageWorkspace(nullptr, H, W, bin).bytes;
}

int gpsa_image_select_count_u8(const unsigned char* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                               int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                               void* stream) {
  return gpsa::image_select_count(img, H, W, C, bin, has_bg, bg, has_bbox, bbox, workspace, workspace_bytes,
                                  as_stream(stream));
}

int gpsa_image_select_count_f32(const float* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                                int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                                void* stream) {
  return gpsa::image_select_count(img, H, W, C, bin, has_bg, bg, has_bbox, bbox, workspace, workspace_bytes,
                                  as_stream(stream));
}

int gpsa_image_select_write_u8(const unsigned char* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                               int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                               float* coords, float* pixels, long long capacity, void* stream) {
  return gpsa::image_select_write(img, H, W, C, bin, has_bg, bg, has_bbox, bbox, workspace, workspace_bytes, coords,
                                  pixels, capacity, as_stream(stream));
}

int gpsa_image_select_write_f32(const float* img, long long H, long long W, int C, int bin, int has_bg, float bg,
                                int has_bbox, const double* bbox, void* workspace, long long workspace_bytes,
                                float* coords, float* pixels, long long capacity, void* stream) {
  return gpsa::image_select_write(img, H, W, C, bin, has_bg, bg, has_bbox, bbox, workspace, workspace_bytes, coords,
                                  pixels, capacity, as_stream(stream));
}

int gpsa_image_sample_u8(const unsigned char* img, long long H, long long W, int C, const double* xy, long long n,
                         int order, float fill, float* out, unsigned char* valid, void* stream) {
  return gpsa::image_sample(img, H, W, C, xy, n, order, fill, out, valid, as_stream(stream));
}

int gpsa_image_sample_f32(const float* img, long long H, long long W, int C, const double* xy, long long n, int order,
                          float fill, float* out, unsigned char* valid, void* stream) {
  return gpsa::image_sample(img, H, W, C, xy, n, order, fill, out, valid, as_stream(stream));
}

}  // extern "C"
