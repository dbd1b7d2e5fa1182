// Bubble-condensed assembly of -(a u')' + b u' + c u = f: every element carries the two P1
// functions and the hierarchic bubbles of degree 2 .. p (p = 2, 3, 4), the bubbles are eliminated element by element,
// and what is assembled is again tridiagonal on the nodes -- the bands (diag, sub, sup) of lssvr_p1_assemble_conv and
// the loads of R right-hand sides -- with nodal values of order h^(2p).  tridiag.hip / tridiag_pivot.hip solve them.
//
// Shape functions on t in [0,1], s = 2t - 1:  N_0 = 1 - t, N_1 = t, N_k = (P_k(s) - P_{k-2}(s)) / sqrt(2 (2k - 1)).
// Their values and t-derivatives at the points of the rule are computed once on the host (BubbleTab) and travel as a
// kernel argument, so the device and the host mirror read the same numbers.  Two passes:
//   element pass   a thread per element: K (p+1 x p+1), one elimination of the bubble block, the condensed 2 x 2
//                  matrix S and, case by case, the condensed load pair -> work (plane-major: S00, S01, S10, S11 [ne],
//                  g0 [R][ne], g1 [R][ne])
//   node pass      a thread per node gathers its two elements in a fixed order
// No atomics, no LDS, no scratch, no inline assembly; bitwise reproducible.  Each value comes from one inline routine
// that the host mirror (p1_assemble_bubble_host) calls too: with -ffp-contract=off the two are bit-equal.
// FP64, -ffp-contract=off.
#include "lssvr_device.hpp"
#include "lssvr_kernels.hpp"
#include "lssvr_p1.hpp"

#define LSSVR_BB_HD __host__ __device__ __forceinline__

namespace lssvr {

namespace {

constexpr int kBbBlock = 256;          // threads per workgroup (four waves)
constexpr int kBbMaxBlocks = 16384;    // grid cap of the grid-stride loops

inline unsigned bb_blocks(int64_t n) {
  const int64_t b = (n + kBbBlock - 1) / kBbBlock;
  return (unsigned)(b < 1 ? 1 : (b < kBbMaxBlocks ? b : kBbMaxBlocks));
}

// w[q]: the weights of the rule; N[i][q], D[i][q]: N_i and dN_i/dt at its points (i <= p, q < nquad; the rest zero)
struct BubbleTab {
  double w[5];
  double N[5][5];
  double D[5][5];
};

// Legendre recurrence on the host; d/ds (P_k - P_{k-2}) = (2k - 1) P_{k-1}, so dN_k/dt = sqrt(2 (2k - 1)) P_{k-1}(s)
void bubble_tab(int p, int nquad, const QuadRule& q, BubbleTab& t) {
  t = BubbleTab{};
  for (int k = 0; k < nquad; ++k) {
    const double tt = q.xi[k], s = 2.0 * tt - 1.0;
    double P[5];
    P[0] = 1.0;
    P[1] = s;
    for (int m = 2; m <= 4; ++m) P[m] = ((2 * m - 1) * s * P[m - 1] - (m - 1) * P[m - 2]) / m;
    t.w[k] = q.wt[k];
    t.N[0][k] = 1.0 - tt;
    t.N[1][k] = tt;
    t.D[0][k] = -1.0;
    t.D[1][k] = 1.0;
    for (int m = 2; m <= p; ++m) {
      const double sc = sqrt(2.0 * (2 * m - 1));
      t.N[m][k] = (P[m] - P[m - 2]) / sc;
      t.D[m][k] = sc * P[m - 1];
    }
  }
}

// The condensed matrix of one element of length h; a, b, c: its nquad table values (NULL: a = 1, b = 0, c = 0).  The
// order of every sum (q, j, k ascending unless said otherwise):
//   wa_q = w_q a_q (w_q without a),  wb_q = w_q b_q,  wc_q = w_q c_q
//   A_ij = sum_q (wa_q D_i) D_j,  C_ij = sum_q (wc_q N_i) N_j   for j >= i, mirrored below;  B_ij = sum_q (wb_q N_i) D_j
//   K_ij = (A_ij / h + h C_ij) + B_ij                           without c: C_ij = 0.0; without b: no B term
//   K_bb = L U in place, no pivoting (rows and columns 2 .. p)
//   Z K_bb = K_vb:   W_j = (K_vj - sum_{k<j} W_k U_kj) / U_jj,   Z_j = W_j - sum_{k>j} Z_k L_kj   (j descending)
//   S_vw = ((K_vw - Z_v0 K_2w) - Z_v1 K_3w) - Z_v2 K_4w         S = (S00, S01, S10, S11)
// A zero or non-finite pivot U_jj leaves non-finite entries in Z and S.
template <int P, int NQ>
LSSVR_BB_HD void bubble_matrix(const BubbleTab& t, double h, const double* __restrict__ a,
                               const double* __restrict__ b, const double* __restrict__ c, double (&S)[4],
                               double (&Z)[2][P - 1]) {
  constexpr int N = P + 1, NB = P - 1;
  double wa[NQ], wb[NQ], wc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    wa[q] = a ? t.w[q] * a[q] : t.w[q];
    wb[q] = b ? t.w[q] * b[q] : 0.0;
    wc[q] = c ? t.w[q] * c[q] : 0.0;
  }
  double K[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = i; j < N; ++j) {
      double A = 0.0, C = 0.0;
#pragma unroll
      for (int q = 0; q < NQ; ++q) A += (wa[q] * t.D[i][q]) * t.D[j][q];
      if (c) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) C += (wc[q] * t.N[i][q]) * t.N[j][q];
      }
      K[i][j] = A / h + h * C;
      K[j][i] = K[i][j];
    }
  }
  if (b) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double B = 0.0;
#pragma unroll
        for (int q = 0; q < NQ; ++q) B += (wb[q] * t.N[i][q]) * t.D[j][q];
        K[i][j] = K[i][j] + B;
      }
    }
  }
  // K_bb = L U (L unit lower, stored below the diagonal)
#pragma unroll
  for (int k = 0; k < NB; ++k) {
#pragma unroll
    for (int i = k + 1; i < NB; ++i) {
      const double l = K[2 + i][2 + k] / K[2 + k][2 + k];
      K[2 + i][2 + k] = l;
#pragma unroll
      for (int j = k + 1; j < NB; ++j) K[2 + i][2 + j] = K[2 + i][2 + j] - l * K[2 + k][2 + j];
    }
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      double s = K[v][2 + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - Z[v][k] * K[2 + k][2 + j];
      Z[v][j] = s / K[2 + j][2 + j];
    }
#pragma unroll
    for (int j = NB - 2; j >= 0; --j) {
      double s = Z[v][j];
#pragma unroll
      for (int k = j + 1; k < NB; ++k) s = s - Z[v][k] * K[2 + k][2 + j];
      Z[v][j] = s;
    }
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      double s = K[v][w];
#pragma unroll
      for (int j = 0; j < NB; ++j) s = s - Z[v][j] * K[2 + j][w];
      S[2 * v + w] = s;
    }
  }
}

// The condensed load pair of one case; f: its nquad table values.
//   g_i = h sum_q N_i (w_q f_q),      out_v = ((g_v - Z_v0 g_2) - Z_v1 g_3) - Z_v2 g_4
template <int P, int NQ>
LSSVR_BB_HD void bubble_load(const BubbleTab& t, double h, const double* __restrict__ f, const double (&Z)[2][P - 1],
                             double& g0, double& g1) {
  constexpr int N = P + 1, NB = P - 1;
  double fq[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) fq[q] = t.w[q] * f[q];
  double g[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) s += t.N[i][q] * fq[q];
    g[i] = h * s;
  }
  double o[2];
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    double s = g[v];
#pragma unroll
    for (int j = 0; j < NB; ++j) s = s - Z[v][j] * g[2 + j];
    o[v] = s;
  }
  g0 = o[0];
  g1 = o[1];
}

// element e of the element pass: everything it writes
template <int P, int NQ>
LSSVR_BB_HD void bubble_element(const P1BubbleArgs& p, const BubbleTab& t, int64_t e) {
  const double h = p.x[e + 1] - p.x[e];
  const int64_t row = e * NQ;
  double S[4], Z[2][P - 1];
  bubble_matrix<P, NQ>(t, h, p.a_quad ? p.a_quad + row : nullptr, p.b_quad ? p.b_quad + row : nullptr,
                       p.c_quad ? p.c_quad + row : nullptr, S, Z);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    p.work[k * p.ne + e] = S[k];
    if (p.kloc4) p.kloc4[4 * e + k] = S[k];
  }
  double* G = p.work + 4 * p.ne;
  for (int r = 0; r < p.R; ++r) {
    double g0, g1;
    bubble_load<P, NQ>(t, h, p.rhs_quad + ((int64_t)r * p.ne + e) * NQ, Z, g0, g1);
    G[(int64_t)r * p.ne + e] = g0;
    G[((int64_t)p.R + r) * p.ne + e] = g1;
    if (p.floc) {
      p.floc[2 * ((int64_t)r * p.ne + e)] = g0;
      p.floc[2 * ((int64_t)r * p.ne + e) + 1] = g1;
    }
  }
}

// node i of the node pass:  diag = S11[i-1] + S00[i],  sub[i] = S10[i],  sup[i] = S01[i],  load[r] = g1[r][i-1] +
// g0[r][i]; at nodes 0 and ne the term of the missing element is left out, not added as 0
LSSVR_BB_HD void bubble_node(const P1BubbleArgs& p, int64_t i) {
  const int64_t ne = p.ne;
  const double* S = p.work;
  const double* G = p.work + 4 * ne;
  if (i < ne) {
    p.sup[i] = S[ne + i];
    p.sub[i] = S[2 * ne + i];
  }
  p.diag[i] = i == 0 ? S[0] : (i == ne ? S[3 * ne + i - 1] : S[3 * ne + i - 1] + S[i]);
  for (int r = 0; r < p.R; ++r) {
    const double* g0 = G + (int64_t)r * ne;
    const double* g1 = G + ((int64_t)p.R + r) * ne;
    p.load[(int64_t)r * (ne + 1) + i] = i == 0 ? g0[0] : (i == ne ? g1[i - 1] : g1[i - 1] + g0[i]);
  }
}

template <int P, int NQ>
__global__ __launch_bounds__(kBbBlock) void p1_bubble_element_kernel(P1BubbleArgs p, BubbleTab t) {
  const int64_t stride = (int64_t)gridDim.x * kBbBlock;
  for (int64_t e = (int64_t)blockIdx.x * kBbBlock + threadIdx.x; e < p.ne; e += stride) bubble_element<P, NQ>(p, t, e);
}

__global__ __launch_bounds__(kBbBlock) void p1_bubble_node_kernel(P1BubbleArgs p) {
  const int64_t stride = (int64_t)gridDim.x * kBbBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBbBlock + threadIdx.x; i <= p.ne; i += stride) bubble_node(p, i);
}

template <int P, int NQ>
void bubble_elements_host(const P1BubbleArgs& p, const BubbleTab& t) {
  for (int64_t e = 0; e < p.ne; ++e) bubble_element<P, NQ>(p, t, e);
}

// the (order, nquad) pairs that exist: nquad = order + 1 .. 5
#define LSSVR_BB_DISPATCH(CALL)                     \
  switch (a.order * 8 + a.nquad) {                  \
    case 2 * 8 + 3: CALL(2, 3); break;              \
    case 2 * 8 + 4: CALL(2, 4); break;              \
    case 2 * 8 + 5: CALL(2, 5); break;              \
    case 3 * 8 + 4: CALL(3, 4); break;              \
    case 3 * 8 + 5: CALL(3, 5); break;              \
    case 4 * 8 + 5: CALL(4, 5); break;              \
    default: return false;                          \
  }

bool bubble_setup(const P1BubbleArgs& a, BubbleTab& t) {
  QuadRule q;
  if (a.order < 2 || a.order > 4 || a.nquad < a.order + 1 || !quad_rule(a.nquad, q)) return false;
  bubble_tab(a.order, a.nquad, q, t);
  return true;
}

}  // namespace

int64_t p1_bubble_work_bytes(int64_t ne, int R) { return (4 + 2 * (int64_t)R) * ne * (int64_t)sizeof(double); }

hipError_t p1_assemble_bubble(const P1BubbleArgs& a, hipStream_t s) {
  BubbleTab t;
  if (!bubble_setup(a, t)) return hipErrorInvalidValue;
  const dim3 grid(bb_blocks(a.ne)), block(kBbBlock);
  auto launch = [&]() -> bool {
#define LSSVR_BB_LAUNCH(P, NQ) hipLaunchKernelGGL((p1_bubble_element_kernel<P, NQ>), grid, block, 0, s, a, t)
    LSSVR_BB_DISPATCH(LSSVR_BB_LAUNCH)
#undef LSSVR_BB_LAUNCH
    return true;
  };
  if (!launch()) return hipErrorInvalidValue;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(p1_bubble_node_kernel, dim3(bb_blocks(a.ne + 1)), block, 0, s, a);
  return hipGetLastError();
}

bool p1_assemble_bubble_host(const P1BubbleArgs& a) {
  BubbleTab t;
  if (!bubble_setup(a, t)) return false;
  auto run = [&]() -> bool {
#define LSSVR_BB_RUN(P, NQ) bubble_elements_host<P, NQ>(a, t)
    LSSVR_BB_DISPATCH(LSSVR_BB_RUN)
#undef LSSVR_BB_RUN
    return true;
  };
  if (!run()) return false;
  for (int64_t i = 0; i <= a.ne; ++i) bubble_node(a, i);
  return true;
}

}  // namespace lssvr
