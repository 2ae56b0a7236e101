// ba_chol.hip -- dense fp64 factor-and-solve on the device: A x = b for a symmetric positive definite
// A through a blocked right-looking Cholesky A = L L^T with panels of kCholNB = 96 columns.  Layout: ba_chol.h.
//
// Per panel k, two plain launches:
//   k_chol_panel   factors the 96 x 96 diagonal block and solves the rows below against it (X L_kk^T = A), one
//                  workgroup per 32 rows.  Every workgroup carries the diagonal block along with its own rows through
//                  the same 96 column steps, so each of them derives the same L_kk in the same operation order, bit
//                  for bit, and no second launch and no wait between workgroups is needed.  The launch never writes
//                  the diagonal block it reads (a workgroup that starts late must still find A_kk there): workgroup
//                  0 stores L_kk into the factor rows behind the matrix, which only k_chol_back reads.
//   k_chol_update  A_ij -= L_ik L_jk^T over the 96 x 96 tiles i >= j > k on the fp64 matrix pipe.
// The right-hand side is row 0 of one more block of rows, so the panel solve and the update turn it into y = L^-1 b
// on the way.  L^T x = y then runs from the last panel to the first (k_chol_back): x_j from the diagonal block, then
// y_k -= L_jk^T x_j for all k < j, one output column per thread over the contiguous rows of block j.
//
// No atomics, no grid barrier, no spinning: a pivot that is <= 0 or not finite sets status in device memory, every
// later kernel reads it first and returns.  Every sum runs in an order fixed by n alone.
#include <cfloat>

#include "ba_chol.h"

namespace pcd {

constexpr int kNB = kCholNB;
constexpr int kPanelTile = 32;          // rows below the diagonal block per workgroup of k_chol_panel
constexpr int kPanelCG = 4;             // threads per row; thread (R, cg) holds columns cg + 4 m, m < 24
constexpr int kPanelCols = kNB / kPanelCG;
constexpr int kPanelThreads = (kNB + kPanelTile) * kPanelCG;   // 512
typedef double chol_f64x4 __attribute__((ext_vector_type(4)));

// Zeros over what the solve reads -- row r of the matrix up to the end of its diagonal tile, the block of the
// right-hand side whole --, the identity on the padding, the status record of a fresh solve.  The upper tiles and the
// factor rows are never read before they are written.  thread = column, blockIdx.y = row.
__global__ __launch_bounds__(256) void k_chol_clear(double* __restrict__ A, int n, int np,
                                                    pcd_ba_chol_info* __restrict__ st) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  for (int r = blockIdx.y; r < np + kNB; r += gridDim.y) {
    const int lim = r < np ? (r / kNB + 1) * kNB : np;
    if (c < lim) A[(size_t)r * np + c] = (r == c && r >= n) ? 1.0 : 0.0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    pcd_ba_chol_info o;
    o.status = PCD_CHOL_OK; o.failed_column = -1; o.n = n; o.n_padded = np; o.panels = np / kNB;
    o.min_pivot = __longlong_as_double(0x7FF0000000000000ll); o.max_pivot = 0.0;
    *st = o;
  }
}

// lower triangle of the caller's S and the right-hand side row; thread = column, blockIdx.y strides the rows
__global__ __launch_bounds__(256) void k_chol_fill_dense(double* __restrict__ A, int n, int np,
                                                         const double* __restrict__ S, const double* __restrict__ rhs) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  for (int r = blockIdx.y; r < n; r += gridDim.y)
    if (c <= r) A[(size_t)r * np + c] = S[(size_t)r * n + c];
  if (blockIdx.y == 0) A[(size_t)np * np + c] = rhs[c];
}

// Panel k: thread (R, cg) holds 24 columns of one row in registers: R < 96 is row R of the diagonal block, R >= 96
// row R - 96 of the workgroup's own 32 rows below it.  Column step j: the owners of column j put their entries into
// LDS; after the barrier everyone reads the pivot, scales by 1 / sqrt(pivot) -- the stored factor and the factor used
// in the updates are the same product, so L is what was subtracted -- and subtracts l_R l_c from its columns c > j.
// One barrier per step (two column buffers).  Rows of the diagonal block above the pivot keep updating columns of the
// upper triangle that nobody reads; their finished entries c <= R are not touched any more.
__global__ __launch_bounds__(kPanelThreads) void k_chol_panel(double* __restrict__ A, int np, int n, int k,
                                                              pcd_ba_chol_info* st) {
  __shared__ double s_col[2][kNB + kPanelTile];
  if (st->status != PCD_CHOL_OK) return;
  const int cg = threadIdx.x & (kPanelCG - 1), R = threadIdx.x >> 2;
  const size_t ld = (size_t)np;
  const int col0 = k * kNB;
  const bool below = R >= kNB;
  const size_t grow = below ? (size_t)col0 + kNB + (size_t)kPanelTile * blockIdx.x + (R - kNB) : (size_t)col0 + R;
  double* row = A + grow * ld + col0;
  double a[kPanelCols];
#pragma unroll
  for (int m = 0; m < kPanelCols; ++m) {
    const int c = cg + kPanelCG * m;
    a[m] = (below || c <= R) ? row[c] : 0.0;
  }
  const bool keeper = blockIdx.x == 0 && threadIdx.x == 0;   // keeps the pivot record
  double pmin = __longlong_as_double(0x7FF0000000000000ll), pmax = 0.0;
#pragma unroll
  for (int jm = 0; jm < kPanelCols; ++jm) {
#pragma unroll 1
    for (int jj = 0; jj < kPanelCG; ++jj) {
      const int j = kPanelCG * jm + jj;
      double* cb = s_col[j & 1];
      if (cg == jj) cb[R] = a[jm];
      __syncthreads();
      const double piv = cb[j];
      if (!(piv > 0.0 && piv <= DBL_MAX)) {   // the same value in every thread of every workgroup
        if (keeper) {
          st->min_pivot = fmin(st->min_pivot, pmin); st->max_pivot = fmax(st->max_pivot, pmax);
          st->failed_column = col0 + j; st->status = PCD_CHOL_NOT_POSITIVE_DEFINITE;
        }
        return;
      }
      const double rinv = 1.0 / sqrt(piv);
      if (col0 + j < n) { const double ljj = piv * rinv; pmin = fmin(pmin, ljj); pmax = fmax(pmax, ljj); }   // L_jj as stored
      const double lR = cb[R] * rinv;
#pragma unroll
      for (int m = jm; m < kPanelCols; ++m) {
        const int c = cg + kPanelCG * m;
        if (m > jm || cg > jj) a[m] -= lR * (cb[c] * rinv);
        else if (cg == jj) a[m] = lR;
      }
    }
  }
  // own rows in place; L_kk (workgroup 0) into the factor rows, never over the A_kk the other workgroups read
  double* out = below ? row : A + ((size_t)np + kNB + R) * ld + col0;
  if (below || blockIdx.x == 0) {
#pragma unroll
    for (int m = 0; m < kPanelCols; ++m) {
      const int c = cg + kPanelCG * m;
      if (below || c <= R) out[c] = a[m];
    }
  }
  if (keeper) { st->min_pivot = fmin(st->min_pivot, pmin); st->max_pivot = fmax(st->max_pivot, pmax); }
}

// Trailing update behind panel k: workgroup = tile (I, J) of 96 x 96, I >= J, counted from block k + 1 (I may be the
// block of the right-hand side row), m (m + 1) / 2 + m of them; wavefront = 48 x 48 of it as 3 x 3 matrix-pipe tiles.  The accumulators start
// from A_ij and the A operand is negated, so an entry is one chain A_ij - l_i0 l_j0 - l_i1 l_j1 - ... over the panel's
// 96 columns.  Operands come straight from the panel (lane l: row l & 15, column 4 step + (l >> 4)), the next step's
// six loads are issued ahead of the nine instructions of the current one.  The upper-right 48 x 48 of a diagonal tile
// is skipped: nobody reads the upper triangle.
__global__ __launch_bounds__(256) void k_chol_update(double* __restrict__ A, int np, int k,
                                                     const pcd_ba_chol_info* __restrict__ st) {
  if (st->status != PCD_CHOL_OK) return;
  // tile blockIdx.x of the lower triangle, row by row: row I starts at I (I + 1) / 2 and holds J = 0 .. I; the last
  // row, the right-hand side's, has no diagonal tile and is simply cut short by the grid
  int I = (int)((sqrtf(8.0f * (float)blockIdx.x + 1.0f) - 1.0f) * 0.5f);
  while ((unsigned)(I + 1) * (unsigned)(I + 2) / 2 <= blockIdx.x) ++I;
  while ((unsigned)I * (unsigned)(I + 1) / 2 > blockIdx.x) --I;
  const int J = (int)(blockIdx.x - (unsigned)I * (unsigned)(I + 1) / 2);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wr = w >> 1, wc = w & 1;
  if (I == J && wc > wr) return;
  const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
  const size_t ld = (size_t)np;
  const size_t rowI = (size_t)(k + 1 + I) * kNB + 48 * wr, rowJ = (size_t)(k + 1 + J) * kNB + 48 * wc;
  const double* Li = A + (rowI + r16) * ld + (size_t)k * kNB + q;
  const double* Lj = A + (rowJ + r16) * ld + (size_t)k * kNB + q;
  double* C = A + (rowI + q) * ld + rowJ + r16;   // register g of tile (i, j): row 16 i + q + 4 g, column 16 j + r16
  chol_f64x4 acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[i][j][g] = C[(size_t)(16 * i + 4 * g) * ld + 16 * j];
  double a0[3], b0[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { a0[i] = Li[(size_t)(16 * i) * ld]; b0[i] = Lj[(size_t)(16 * i) * ld]; }
#pragma unroll
  for (int ks = 0; ks < kNB / 4; ++ks) {
    double a1[3] = {0.0, 0.0, 0.0}, b1[3] = {0.0, 0.0, 0.0};
    if (ks + 1 < kNB / 4) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        a1[i] = Li[(size_t)(16 * i) * ld + 4 * (ks + 1)]; b1[i] = Lj[(size_t)(16 * i) * ld + 4 * (ks + 1)];
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) { a0[i] = a1[i]; b0[i] = b1[i]; }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) C[(size_t)(16 * i + 4 * g) * ld + 16 * j] = acc[i][j][g];
}

// Backward solve, panel j: every workgroup solves L_jj^T x_j = y_j from the diagonal block in LDS (the same 96 steps
// everywhere), workgroup 0 stores x_j; then thread = column c < 96 j: y_c -= sum_r L[96 j + r][c] x_j[r], r ascending.
__global__ __launch_bounds__(256) void k_chol_back(double* __restrict__ A, int np, int j,
                                                   const pcd_ba_chol_info* __restrict__ st) {
  __shared__ double s_L[kNB * kNB];
  __shared__ double s_x[kNB];
  if (st->status != PCD_CHOL_OK) return;
  const size_t ld = (size_t)np;
  const int t = threadIdx.x;
  const double* Lrows = A + (size_t)j * kNB * ld;   // the rows of block j
  const double* Ljj = A + (ld + kNB) * ld + (size_t)j * kNB;   // its diagonal factor, in the factor rows
  for (int e = t; e < kNB * kNB; e += 256) {
    const int r = e / kNB, c = e - kNB * (e / kNB);
    s_L[e] = c <= r ? Ljj[(size_t)r * ld + c] : 0.0;
  }
  double* y = A + ld * ld;
  double* x = y + ld;
  double v = t < kNB ? y[(size_t)j * kNB + t] : 0.0;
  __syncthreads();
  for (int r = kNB - 1; r >= 0; --r) {
    if (t == r) s_x[r] = v / s_L[r * kNB + r];
    __syncthreads();
    if (t < r) v -= s_L[r * kNB + t] * s_x[r];
  }
  if (blockIdx.x == 0 && t < kNB) x[(size_t)j * kNB + t] = s_x[t];
  const int c = blockIdx.x * 256 + t;
  if (c < j * kNB) {
    double acc = y[c];
    const double* col = Lrows + c;
#pragma unroll 8
    for (int r = 0; r < kNB; ++r) acc -= col[(size_t)r * ld] * s_x[r];
    y[c] = acc;
  }
}

// x (or zeros after a failed factorisation) to the caller, the status record if asked for
__global__ __launch_bounds__(256) void k_chol_finish(const double* __restrict__ A, int np, int n,
                                                     const pcd_ba_chol_info* __restrict__ st, double* __restrict__ x,
                                                     pcd_ba_chol_info* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool ok = st->status == PCD_CHOL_OK;
  if (x && i < n) x[i] = ok ? A[((size_t)np + 1) * np + i] : 0.0;
  if (i == 0 && info) *info = *st;
}

void chol_begin(double* A, int n, pcd_ba_chol_info* status, hipStream_t s) {
  const int np = chol_padded(n);
  hipLaunchKernelGGL(k_chol_clear, dim3(div_up((uint64_t)np, 256), (unsigned)std::min(np + kNB, 65535)), dim3(256), 0, s,
                     A, n, np, status);
}

void chol_fill_dense(double* A, int n, const double* S, const double* rhs, hipStream_t s) {
  hipLaunchKernelGGL(k_chol_fill_dense, dim3(div_up((uint64_t)n, 256), (unsigned)std::min(n, 65535)), dim3(256), 0, s,
                     A, n, chol_padded(n), S, rhs);
}

void chol_factor_solve(double* A, int n, pcd_ba_chol_info* status, double* x, pcd_ba_chol_info* info_out, hipStream_t s) {
  const int np = chol_padded(n), nb = np / kNB;
  for (int k = 0; k < nb; ++k) {
    const int m = nb - 1 - k;   // blocks behind the panel; the right-hand side's 32 rows make one more row tile
    hipLaunchKernelGGL(k_chol_panel, dim3((kNB / kPanelTile) * m + 1), dim3(kPanelThreads), 0, s, A, np, n, k, status);
    if (m) hipLaunchKernelGGL(k_chol_update, dim3((unsigned)m * (m + 1) / 2 + m), dim3(256), 0, s, A, np, k, status);
  }
  for (int j = nb - 1; j >= 0; --j)
    hipLaunchKernelGGL(k_chol_back, dim3(std::max(1u, div_up((uint64_t)j * kNB, 256))), dim3(256), 0, s, A, np, j, status);
  hipLaunchKernelGGL(k_chol_finish, dim3(std::max(1u, div_up((uint64_t)n, 256))), dim3(256), 0, s, A, np, n, status, x,
                     info_out);
}

}  // namespace pcd
