// Polygon rasteriser for MI355X (gfx950): PIL.ImageDraw.polygon's scanline fill; C ABI in include/dspn_polygon.h.
//
// One wave per (polygon, row).  Lanes stride over the polygon's edges; each active edge contributes its crossing
// (float32 multiply, then float32 add: the two roundings of the host rule, never an FMA), twice where it ends on the
// row, or the corner entry the host put in the table.  Ballot + popcount give every lane its slots, so the entries of a
// row land in one array: LDS while they fit, the job's slice of a global scratch buffer when they do not.  The wave
// rank-sorts them (n^2 / 64 compares; a row of a street scene has 2 to 8 entries), takes them in pairs and paints each
// span with lanes striding over its pixels: atomicMax of the polygon's order, so the last polygon of the file owns the
// pixel whatever the order in which waves run.  Pillow's running x_pos only keeps the spans of one row from being
// painted twice; with an idempotent store the union of the spans is the same set of pixels.
#include "dspn_common.h"
#include "../../include/dspn_polygon.h"

namespace {

constexpr int kWave = 64;
constexpr int kWaveEntries = 256;        // entries of a row kept in LDS (twice: unsorted and sorted)

__device__ __forceinline__ int round_half_up(float f) {
  return (int)(f >= 0.0f ? floorf(__fadd_rn(f, 0.5f)) : -floorf(__fadd_rn(fabsf(f), 0.5f)));
}
__device__ __forceinline__ int round_half_down(float f) {
  return (int)(f >= 0.0f ? ceilf(__fadd_rn(f, -0.5f)) : -ceilf(__fadd_rn(fabsf(f), -0.5f)));
}

__device__ __forceinline__ void paint(int *row, int W, int xa, int xb, int order, int lane) {
  xa = max(xa, 0);
  xb = min(xb, W - 1);
  for (int x = xa + lane; x <= xb; x += kWave) atomicMax(row + x, order);
}

__global__ __launch_bounds__(kWave) void polygon_rows_kernel(const int4 *__restrict__ edges, int E,
                                                              const int4 *__restrict__ polys, int P,
                                                              const int *__restrict__ jobs, int J, float *scratch,
                                                              long long scratch_floats, int *owner, int B, int H, int W,
                                                              int *spill_count) {
  __shared__ float lds[2 * kWaveEntries];
  const int job = blockIdx.x, lane = threadIdx.x;
  if (job >= J) return;
  const int p = jobs[job * 5], y = jobs[job * 5 + 1], last_row = jobs[job * 5 + 2], cap = jobs[job * 5 + 3];
  const long long off = jobs[job * 5 + 4];
  if (p < 0 || p >= P || y < 0 || y >= H || cap < 0) return;
  const int4 pg = polys[p];
  const int e0 = pg.x, e1 = pg.y, image = pg.z, order = pg.w;
  if (e0 < 0 || e1 > E || e0 > e1 || image < 0 || image >= B) return;
  float *xx = lds;
  if (cap > kWaveEntries) {
    if (off < 0 || off + 2LL * cap > scratch_floats) return;
    xx = scratch + off;
    if (lane == 0 && spill_count) atomicAdd(spill_count, 1);
  }
  float *sorted = xx + cap;
  int *row = owner + ((long long)image * H + y) * W;
  const unsigned long long below = (1ull << lane) - 1ull;

  int n = 0;
  for (int base = e0; base < e1; base += kWave) {
    const int e = base + lane;
    int x0 = 0, y0 = 0, ymin = 1, ymax = 0, x1 = 0;
    float dx = 0.0f, top = 0.0f, bot = 0.0f;
    if (e < e1) {
      const int4 a = edges[2 * (long long)e], b = edges[2 * (long long)e + 1];
      x0 = a.x; y0 = a.y; ymin = a.z; ymax = a.w;
      dx = __int_as_float(b.x); top = __int_as_float(b.y); bot = __int_as_float(b.z); x1 = b.w;
    }
    const bool flat = ymin == ymax;
    unsigned long long hmask = __ballot(flat && ymin == y);
    while (hmask) {                                  // horizontal edges paint their own span
      const int src = __ffsll((long long)hmask) - 1;
      hmask &= hmask - 1;
      const int xa = __shfl(x0, src), xb = __shfl(x1, src);
      paint(row, W, min(xa, xb), max(xa, xb), order, lane);
    }
    const bool active = !flat && ymin <= y && y <= ymax;
    const bool twice = active && y == ymax && y < last_row;
    float x = __fadd_rn(__fmul_rn((float)(y - y0), dx), (float)x0);
    if (active && !twice) {
      if (y == ymin && y < last_row) { if (top == top) x = top; }
      else if (y == ymax && y == last_row) { if (bot == bot) x = bot; }
    }
    const unsigned long long m1 = __ballot(active), m2 = __ballot(twice);
    const int pos = n + __popcll(m1 & below) + __popcll(m2 & below);
    if (active && pos < cap) xx[pos] = x;
    if (twice && pos + 1 < cap) xx[pos + 1] = x;
    n += __popcll(m1) + __popcll(m2);
  }
  n = min(n, cap);
  __syncthreads();
  for (int i = lane; i < n; i += kWave) {           // rank sort: ties keep their order of entry
    const float v = xx[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float u = xx[j];
      rank += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    sorted[rank] = v;
  }
  __syncthreads();
  for (int i = 1; i < n; i += 2)
    paint(row, W, round_half_up(sorted[i - 1]), round_half_down(sorted[i]), order, lane);
}

constexpr int kResolveThreads = 256;

__global__ __launch_bounds__(kResolveThreads) void polygon_resolve_kernel(const int *__restrict__ owner, long long total,
                                                                         long long plane, int B,
                                                                         const int4 *__restrict__ table, int T,
                                                                         const int *__restrict__ table_offset,
                                                                         unsigned char *label, unsigned char *label_train,
                                                                         int *inst, int *inst_train) {
  const long long step = (long long)gridDim.x * kResolveThreads;
  for (long long i = (long long)blockIdx.x * kResolveThreads + threadIdx.x; i < total; i += step) {
    const int b = (int)(i / plane);
    const long long t = (long long)table_offset[b] + owner[i];
    if (t < 0 || t >= T) continue;
    const int4 v = table[t];
    if (label) label[i] = (unsigned char)v.x;
    if (label_train) label_train[i] = (unsigned char)v.y;
    if (inst) inst[i] = v.z;
    if (inst_train) inst_train[i] = v.w;
  }
}

}  // namespace

extern "C" {

int dspn_polygon_wave_entries(void) { return kWaveEntries; }

int dspn_polygon_rasterize(const int *edges_dev, int E, const int *polys_dev, int P, const int *jobs_dev, int J,
                           float *scratch_dev, long long scratch_floats, int *owner_dev, int B, int H, int W,
                           int *spill_count_dev, void *stream) {
  DSPN_REQUIRE(E >= 0 && P >= 0 && J >= 0 && B >= 0, "polygon_rasterize: negative count");
  DSPN_REQUIRE(H > 0 && W > 0, "polygon_rasterize: H and W must be > 0");
  DSPN_REQUIRE(scratch_floats >= 0 && (scratch_floats == 0 || scratch_dev), "polygon_rasterize: scratch size without a buffer");
  if (J == 0 || B == 0) return 0;
  DSPN_REQUIRE(edges_dev || E == 0, "polygon_rasterize: null edge table");
  DSPN_REQUIRE(polys_dev && jobs_dev && owner_dev, "polygon_rasterize: null pointer");
  hipLaunchKernelGGL(polygon_rows_kernel, dim3(J), dim3(kWave), 0, (hipStream_t)stream, (const int4 *)edges_dev, E,
                     (const int4 *)polys_dev, P, jobs_dev, J, scratch_dev, scratch_floats, owner_dev, B, H, W,
                     spill_count_dev);
  return dspn::check_launch("polygon_rasterize");
}

int dspn_polygon_resolve(const int *owner_dev, int B, int H, int W, const int *table_dev, int T,
                         const int *table_offset_dev, unsigned char *label_dev, unsigned char *label_train_dev,
                         int *inst_dev, int *inst_train_dev, void *stream) {
  DSPN_REQUIRE(B >= 0 && T >= 0, "polygon_resolve: negative count");
  DSPN_REQUIRE(H > 0 && W > 0, "polygon_resolve: H and W must be > 0");
  if (B == 0) return 0;
  DSPN_REQUIRE(owner_dev && table_dev && table_offset_dev, "polygon_resolve: null pointer");
  const long long plane = (long long)H * W, total = plane * B;
  const long long blocks = (total + kResolveThreads - 1) / kResolveThreads;
  hipLaunchKernelGGL(polygon_resolve_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kResolveThreads), 0,
                     (hipStream_t)stream, owner_dev, total, plane, B, (const int4 *)table_dev, T, table_offset_dev,
                     label_dev, label_train_dev, inst_dev, inst_train_dev);
  return dspn::check_launch("polygon_resolve");
}

}  // extern "C"
