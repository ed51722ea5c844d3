// libcatint_modes (include/catint_modes.h): the relaxation modes of a stationary state of the physical mode -- per operating point a
// subspace iteration on A = J^-1 S, every pass one block-tridiagonal solve J W = S Q with the subspace as right-hand sides and the
// Rayleigh-Ritz matrices of the pass -- formed on the device from the state a pnp_handle holds there.  It shares no code with the
// Newton kernels.  The rows of the stationary Jacobian, the team mapping, the walk from block row to block row and the host code around
// the launch are those of ../pnp_team.h (as for response/catresp.hip, couple/catcpl.hip and sens/catsens.hip; the Gauss-Jordan step
// stands in the row loop in the same words as there); here are the right-hand sides S Q, their carriage through the walk (as
// catsens.hip), the records and the substitution towards the bulk (as the profile instances of catresp.hip), and the iteration around
// them: the inner products and the Gram-Schmidt update.
// gfx950 / MI355X only.
//
// Mapping, two phases that alternate inside one launch (systems are independent: a persistent grid, no grid-wide synchronisation):
// TEAM phase (pnp_team.h): a team of NB = N + 1 adjacent lanes per system, 64 / NB systems per wave.  Lane r owns row r of
//   [D'_i | L_i | G_i], G_i the PC carried columns.  After the Gauss-Jordan of row i, T_i and y_i = D'_i^-1 g'_i go to the team through
//   LDS and to the system's workspace slot, and row i-1 forms g'_{i-1} = (S Q)_{i-1} - U_{i-1} y_i.  At the wall the carried columns
//   hold w_0; then the same lanes substitute w_i = y_i - T_i w_{i-1} towards the bulk, each lane reading back the rows it wrote, and
//   w_i replaces y_i in the slot.
// WAVE phase: the whole wave works on one system of the group at a time.  An entry e = i NB + r of a column (grid point i, unknown r)
//   belongs to lane e mod 64; its PC columns lie side by side (64 bytes), so a wave reads consecutive kilobytes.  Sums over the entries
//   are formed per lane in ascending e, then across the wave by the DPP scan of ../pnp_wave.h: an order that depends on nothing but nx
//   and NB.  Between the phases the wave's stores are made visible to its other lanes by a workgroup-scope fence.
// The elimination is repeated in every pass: nothing of the factorisation is kept but the records of the pass in work (DESIGN.md
// section 7l has what that costs).
// Slot of a system: T [nx][NB][NB], X0 [nx][NB][PC], X1 [nx][NB][PC]; pass p reads Q from X(p mod 2) and leaves W, then orth(W), in the
// other.  Columns beyond the subspace size are zero throughout.
// A column's numbers are formed in an order fixed in the source (no implicit contraction).  Results leave through plain vector stores.
#include <cstdlib>
#include <utility>

#include "../../../include/catint_modes.h"
#include "../pnp_team.h"

#pragma clang fp contract(off)

namespace catmodes {

using namespace pnp::team;

constexpr double BREAK2 = CATMODES_BREAKDOWN * CATMODES_BREAKDOWN;

using Table = pnp::team::WallTable;   // the reaction and wall tables of one call

struct KArgs {
  int32_t nx, ldx, nreact, nwall, stern, steric, m, K;
  int64_t nsys;            // selected operating points
  int64_t slot;            // doubles of a system's workspace slot
  const double* c;         // [B][N][ldx]
  const double* phi;       // [B][ldx]
  const int32_t* st;       // [B] solver status
  const int64_t* lanes;    // [n]
  const int32_t* badin;    // [n] 1: an input of the point is not finite
  const double *wgt, *vol; // [nx-1] dx / h_e, [nx] v_i
  const double* sp;        // [NB][SPF]
  const double *kwall, *phiM;   // [B][nwall], [B]
  const double* start;     // [m][NB][nx]
  const Table* tab;
  double *ritz, *gram, *basis;   // device rows; null: not wanted
  int32_t* flags;          // [n]
  double* ws;              // [grid x teams] slots
  Consts k;
};

__host__ __device__ constexpr size_t even_(size_t n) { return (n + 1) & ~(size_t)1; }

// g and dg/dc_s of wall reaction r at the wall state (cs: the driving concentration, 1 for species -1)
__device__ __forceinline__ void wall_law(const Table& tb, int r, double cs, double dphi, double& g, double& dg) {
  const double al = tb.alpha[r];
  const double den = 1.0 / (1.0 + tb.sat[r] * cs);
  const double E = al != 0.0 ? exp(al * dphi) : 1.0;
  g = cs * den * E;
  dg = den * den * E;
}

// g'_{i-1} = r_{i-1} - U_{i-1} y_i, row r0, into G; ym: y_i of the team, whose row r0 the lane still holds in G
template <int NB, int PC>
__device__ __forceinline__ void carry(bool steric, const Lane& ln, const double (&ym)[NB][PC], const double (&Ur)[NB], const double (&rv)[PC],
                                      double (&G)[PC]) {
  constexpr int N = NB - 1;
  if (steric) {
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      double g = rv[m];
#pragma unroll
      for (int s = 0; s < NB; ++s) g = fnma(g, Ur[s], ym[s][m]);
      G[m] = g;
    }
  } else {
    // point ions: U has its diagonal and the phi column
    double ud = 0.0;
#pragma unroll
    for (int s = 0; s < NB; ++s) ud = s == ln.r0 ? Ur[s] : ud;
    const double uN = ln.isP ? 0.0 : Ur[N];
#pragma unroll
    for (int m = 0; m < PC; ++m) {
      double g = fnma(rv[m], ud, G[m]);
      G[m] = fnma(g, uN, ym[N][m]);
    }
  }
}

// ---- the wave phase ----------------------------------------------------------------------------------------------------------------
// what one lane stored to the workspace becomes visible to the other lanes of its wave (one wave per workgroup)
__device__ __forceinline__ void global_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int PC>
__device__ __forceinline__ void load_entry(const double* X, int e, double (&v)[PC]) {
  const pnp::d2* p = reinterpret_cast<const pnp::d2*>(X + (size_t)e * PC);
#pragma unroll
  for (int j = 0; j < PC / 2; ++j) {
    const pnp::d2 t = p[j];
    v[2 * j] = t.x, v[2 * j + 1] = t.y;
  }
}

template <int PC>
__device__ __forceinline__ void store_entry(double* X, int e, const double (&v)[PC]) {
  pnp::d2* p = reinterpret_cast<pnp::d2*>(X + (size_t)e * PC);
#pragma unroll
  for (int j = 0; j < PC / 2; ++j) {
    pnp::d2 t;
    t.x = v[2 * j], t.y = v[2 * j + 1];
    p[j] = t;
  }
}

// the sums over the wave of every acc[j], to every lane: the scan's total leaves lane 63 through LDS (red: NV doubles)
template <int NV>
__device__ __forceinline__ void wave_totals(double (&acc)[NV], double* red, int lane) {
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const double s = pnp::wave_scan_incl_bc(acc[j]);
    if (lane == 63) red[j] = s;
  }
  pnp::lds_sync();
#pragma unroll
  for (int j = 0; j < NV; ++j) acc[j] = red[j];
  pnp::lds_sync();
}

// the start vectors into a slot's layout; columns beyond m are zero
template <int NB, int PC>
__device__ __forceinline__ void load_start(const double* start, double* X, int nx, int m, int lane) {
  const int E = nx * NB;
  for (int e = lane; e < E; e += 64) {
    const int i = e / NB, r = e - i * NB;
    double v[PC];
#pragma unroll
    for (int j = 0; j < PC; ++j) v[j] = j < m ? start[((size_t)j * NB + r) * nx + i] : 0.0;
    store_entry<PC>(X, e, v);
  }
}

// step k of orth: q_k = v_k / sqrt(d_kk), v_j <- v_j - (d_kj / d_kk) v_k for j > k, and d_{k+1,j} of the updated columns in the same sweep
template <int PC, int k>
__device__ __forceinline__ void orth_step(double* X, int E, int m, double* red, int lane, const double (&nb)[PC], double (&d)[PC], int& fl) {
  if (k >= m) return;
  constexpr int k1 = k + 1 < PC ? k + 1 : k;
  const double dk = d[k];
  const bool ok = dk > BREAK2 * nb[k];
  fl |= ok ? 0 : 2;
  const double s = ok ? 1.0 / sqrt(dk) : 0.0;
  double f[PC], dn[PC];
#pragma unroll
  for (int j = 0; j < PC; ++j) {
    f[j] = (ok && j > k) ? d[j] / dk : 0.0;
    dn[j] = 0.0;
  }
  for (int e = lane; e < E; e += 64) {
    double v[PC];
    load_entry<PC>(X, e, v);
    const double q = v[k];
#pragma unroll
    for (int j = k + 1; j < PC; ++j) v[j] = fnma(v[j], f[j], q);
    v[k] = q * s;
#pragma unroll
    for (int j = k + 1; j < PC; ++j) dn[j] = fma_(v[k1], v[j], dn[j]);
    store_entry<PC>(X, e, v);
  }
  if (k + 1 < m) {
    wave_totals<PC>(dn, red, lane);
#pragma unroll
    for (int j = 0; j < PC; ++j) d[j] = dn[j];
  }
}

template <int PC, int... Ks>
__device__ __forceinline__ void orth_steps(double* X, int E, int m, double* red, int lane, const double (&nb)[PC], double (&d)[PC], int& fl,
                                           std::integer_sequence<int, Ks...>) {
  (orth_step<PC, Ks>(X, E, m, red, lane, nb, d, fl), ...);
}

// X = orth(X) in place (catint_modes.h: right-looking modified Gram-Schmidt, columns in order).  Every lane reads and writes its own
// entries only.  Returns 1: a non-finite norm, 2: breakdown (the column is zeroed)
template <int PC>
__device__ __forceinline__ int orth(double* X, int E, int m, double* red, int lane) {
  double nb[PC], d[PC];   // |v_j|^2 as the column came in; <v_k, v_j> for the k in work
#pragma unroll
  for (int j = 0; j < PC; ++j) nb[j] = 0.0, d[j] = 0.0;
  for (int e = lane; e < E; e += 64) {
    double v[PC];
    load_entry<PC>(X, e, v);
#pragma unroll
    for (int j = 0; j < PC; ++j) {
      nb[j] = fma_(v[j], v[j], nb[j]);
      d[j] = fma_(v[0], v[j], d[j]);
    }
  }
  wave_totals<PC>(nb, red, lane);
  wave_totals<PC>(d, red, lane);
  int fl = 0;
#pragma unroll
  for (int j = 0; j < PC; ++j) fl |= finite_(nb[j]) ? 0 : 1;
  orth_steps<PC>(X, E, m, red, lane, nb, d, fl, std::make_integer_sequence<int, PC>());
  return fl;
}

// B = Q^T W and G = (W - Q B)^T (W - Q B) of one system into red[0 .. PC PC) and red[PC PC .. 2 PC PC), row-major.  Returns 1 when
// a number is not finite
template <int PC>
__device__ __forceinline__ int rayleigh_ritz(const double* Xq, const double* Xw, int E, double* red, int lane) {
  double Bv[PC * PC];
#pragma unroll
  for (int a = 0; a < PC * PC; ++a) Bv[a] = 0.0;
  for (int e = lane; e < E; e += 64) {
    double q[PC], w[PC];
    load_entry<PC>(Xq, e, q);
    load_entry<PC>(Xw, e, w);
#pragma unroll
    for (int a = 0; a < PC; ++a) {
#pragma unroll
      for (int b = 0; b < PC; ++b) Bv[a * PC + b] = fma_(q[a], w[b], Bv[a * PC + b]);
    }
  }
  wave_totals<PC * PC>(Bv, red, lane);
  double Gv[PC * PC];   // b >= a is formed
#pragma unroll
  for (int a = 0; a < PC * PC; ++a) Gv[a] = 0.0;
  for (int e = lane; e < E; e += 64) {
    double q[PC], w[PC];
    load_entry<PC>(Xq, e, q);
    load_entry<PC>(Xw, e, w);
#pragma unroll
    for (int b = 0; b < PC; ++b) {
#pragma unroll
      for (int a = 0; a < PC; ++a) w[b] = fnma(w[b], q[a], Bv[a * PC + b]);
    }
#pragma unroll
    for (int a = 0; a < PC; ++a) {
#pragma unroll
      for (int b = a; b < PC; ++b) Gv[a * PC + b] = fma_(w[a], w[b], Gv[a * PC + b]);
    }
  }
#pragma unroll
  for (int a = 0; a < PC; ++a) {
#pragma unroll
    for (int b = a; b < PC; ++b) {
      const double s = pnp::wave_scan_incl_bc(Gv[a * PC + b]);
      if (lane == 63) red[PC * PC + a * PC + b] = s, red[PC * PC + b * PC + a] = s;
    }
  }
  pnp::lds_sync();   // (wave_totals left B in red[0 .. PC PC))
  static_assert(2 * PC * PC >= 64 && (2 * PC * PC) % 64 == 0, "every lane checks its share of B and G");
  bool nf = false;
#pragma unroll
  for (int a = 0; a < 2 * PC * PC; a += 64) nf = nf || !finite_(red[a + lane]);
  return __any(nf) ? 1 : 0;
}

template <int NB, int PC>
__global__ __launch_bounds__(64) void modes_kernel(const KArgs A) {
  constexpr int N = NB - 1, TPW = 64 / NB, W = 2 * NB + PC;
  const Lane ln = lane_of<NB>(A.sp);
  const int team = ln.team, r0 = ln.r0, base = ln.base;
  const int lane = threadIdx.x;
  const bool isP = ln.isP;
  const int nx = A.nx, E = nx * NB, msub = A.m;
  const size_t tsz = even_((size_t)E * NB), xsz = (size_t)E * PC;
  const Table& tb = *A.tab;

  __shared__ Ring<NB> ring;
  __shared__ double prow[2][TPW + 1][W];      // the pivot row of an elimination step (two buffers: one wave-level sync per step)
  __shared__ double tmat[TPW + 1][NB][NB];    // T_i
  __shared__ double ymat[TPW + 1][NB][PC];    // y_i
  __shared__ double xb[2][TPW + 1][NB][PC];   // the substitution: w_{i-1} and w_i of the team
  __shared__ double red[2 * PC * PC];         // the wave phase: totals, then B and G of the system in work
  __shared__ int wflag[TPW + 1];              // the wave phase's flags per team (1: not finite, 2: breakdown)

  for (int64_t grp = blockIdx.x; grp * TPW < A.nsys; grp += gridDim.x) {
    const int64_t sys = grp * TPW + team;
    const bool live = team < TPW && sys < A.nsys;
    const int64_t sy = live ? sys : grp * TPW;
    const int64_t b = A.lanes[sy];
    const double* urow = isP ? A.phi + (size_t)b * A.ldx : A.c + ((size_t)b * N + r0) * A.ldx;
    const double phiM = A.phiM[b];
    const int nlive = (int)(A.nsys - grp * TPW < TPW ? A.nsys - grp * TPW : TPW);
    double* const slot0 = A.ws + (size_t)blockIdx.x * TPW * (size_t)A.slot;
    double* const Trec = slot0 + (size_t)(team < TPW ? team : 0) * (size_t)A.slot;
    bool bad = false;

    // ---- Q = orth(start), system by system ----
    for (int t = 0; t < nlive; ++t) {
      double* X = slot0 + (size_t)t * (size_t)A.slot + tsz;
      load_start<NB, PC>(A.start, X, nx, msub, lane);
      const int fl = orth<PC>(X, E, msub, red, lane);
      if (lane == 0) wflag[t] = fl;
    }
    global_sync();

#pragma unroll 1
    for (int pass = 0; pass < A.K; ++pass) {
      const double* Xq = Trec + tsz + (size_t)(pass & 1) * xsz;
      double* Xw = Trec + tsz + (size_t)((pass + 1) & 1) * xsz;

      // ======== team phase: J W = S Q ========
      Window w;
      double c4;
      open<NB>(A, ring, ln, urow, w, c4);

      double Aw[2 * NB];   // [D'_i | L_i], row r0
      double G[PC];        // the carried columns, row r0
      double Ur[NB];       // U_i, row r0
      double rv[PC];

      // row r0 of (S Q)_i, i < nx-1: (dx^2 / D_k) v_i on a species row, 0 on the Poisson row
      const auto row_rhs = [&](int i) {
        const double sv = ln.rs * A.vol[i];
        double q[PC];
#pragma unroll
        for (int m = 0; m < PC; ++m) q[m] = 0.0;
        if (live) load_entry<PC>(Xq, i * NB + r0, q);
#pragma unroll
        for (int m = 0; m < PC; ++m) rv[m] = sel(isP, 0.0, sv * q[m]);
      };
      // the wall table's part of M_0, formed before the row
      const auto wall_matrix = [&](double (&wallM)[NB]) {
        const double* cc = ring[0] + base;
        for (int r = 0; r < A.nwall; ++r) {
          const int s = tb.wspecies[r];
          double g, dg;
          wall_law(tb, r, s >= 0 ? cc[s] : 1.0, phiM - w.C.ph, g, dg);
          const double nk = tb.nu[r][r0] * A.kwall[b * A.nwall + r];
#pragma unroll
          for (int j = 0; j < N; ++j) wallM[j] += j == s ? -nk * dg * ln.dx / ln.Dk : 0.0;
          wallM[N] += nk * tb.alpha[r] * g * ln.dx / ln.Dk;
        }
      };

      first_row<NB, double>(A, tb, ring, ln, w, c4, 0.0, Aw, Ur);
      // y_{nx-1} = 0: the identity rows of the bulk point carry no storage
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        G[m] = 0.0;
        ymat[team][r0][m] = 0.0;
      }
      pnp::lds_sync();
      row_rhs(nx - 2);
      carry<NB, PC>(A.steric, ln, ymat[team], Ur, rv, G);

#pragma unroll 1
      for (int i = nx - 2; i >= 0; --i) {
        const double nxt = i >= 3 ? urow[i - 3] : 0.0;   // the point the row after next needs: used at the end of this block row
        // ---- Gauss-Jordan on [D' | L | G] across the team, no row exchanges ----
#pragma unroll
        for (int p = 0; p < NB; ++p) {
          const bool mine = r0 == p;
          const double piv = Aw[p];
          bad = bad || (mine && !(nonzero(piv) && finite_(piv)));
          const double ip = inv(piv);
          double* pr = prow[p & 1][team];
#pragma unroll
          for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, mul(Aw[j], ip), Aw[j]);
#pragma unroll
          for (int m = 0; m < PC; ++m) G[m] = sel(mine, mul(G[m], ip), G[m]);
          if (mine) {
            pr[p] = piv;
#pragma unroll
            for (int j = p + 1; j < 2 * NB; ++j) pr[j] = Aw[j];
#pragma unroll
            for (int m = 0; m < PC; ++m) pr[2 * NB + m] = G[m];
          }
          pnp::lds_sync();
          // the pivot monitor: what partial pivoting would have checked -- an entry below the pivot beyond the growth limit times the pivot
          bad = bad || (r0 > p && abs2(piv) > GROWTH2 * abs2(pr[p]));
#pragma unroll
          for (int j = p + 1; j < 2 * NB; ++j) Aw[j] = sel(mine, Aw[j], fnma(Aw[j], piv, pr[j]));
#pragma unroll
          for (int m = 0; m < PC; ++m) G[m] = sel(mine, G[m], fnma(G[m], piv, pr[2 * NB + m]));
        }
        if (i == 0) break;
        // ---- T_i = Aw[NB ..], y_i = G: to the team, to the records ----
#pragma unroll
        for (int j = 0; j < NB; ++j) tmat[team][r0][j] = Aw[NB + j];
#pragma unroll
        for (int m = 0; m < PC; ++m) ymat[team][r0][m] = G[m];
        if (live) {
          double* rec = Trec + ((size_t)i * NB + r0) * NB;
#pragma unroll
          for (int j = 0; j < NB; ++j) rec[j] = Aw[NB + j];
          store_entry<PC>(Xw, i * NB + r0, G);
        }
        // ---- row i-1 ----
        shift(A, ln, i, w);
        double wallM[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) wallM[j] = 0.0;
        if (i == 1) wall_matrix(wallM);
        next_row<NB, double>(A, tb, ring, tmat[team], ln, w, i, nxt, 0.0, wallM, Aw, Ur);
        row_rhs(i - 1);
        carry<NB, PC>(A.steric, ln, ymat[team], Ur, rv, G);
      }

      // ---- the wall: w_0[r0] of column m is G[m]; then w_i = y_i - T_i w_{i-1}, the records read back by the lane that wrote them ----
      pnp::lds_sync();   // the last elimination step has read its pivot row
#pragma unroll
      for (int m = 0; m < PC; ++m) {
        xb[0][team][r0][m] = G[m];
        bad = bad || !finite_(G[m]);
      }
      if (live) store_entry<PC>(Xw, r0, G);
      pnp::lds_sync();
#pragma unroll 1
      for (int i = 1; i <= nx - 2; ++i) {
        const double(*xp)[PC] = xb[(i - 1) & 1][team];
        double(*xn)[PC] = xb[i & 1][team];
        double v[PC], tr[NB];
#pragma unroll
        for (int m = 0; m < PC; ++m) v[m] = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) tr[j] = 0.0;
        if (live) {
          const double* rec = Trec + ((size_t)i * NB + r0) * NB;
#pragma unroll
          for (int j = 0; j < NB; ++j) tr[j] = rec[j];
          load_entry<PC>(Xw, i * NB + r0, v);
        }
#pragma unroll
        for (int m = 0; m < PC; ++m) {
#pragma unroll
          for (int j = 0; j < NB; ++j) v[m] = fnma(v[m], tr[j], xp[j][m]);
          bad = bad || !finite_(v[m]);
          xn[r0][m] = v[m];
        }
        pnp::lds_sync();
        if (live) store_entry<PC>(Xw, i * NB + r0, v);
      }
      if (live) {
#pragma unroll
        for (int m = 0; m < PC; ++m) rv[m] = 0.0;
        store_entry<PC>(Xw, (nx - 1) * NB + r0, rv);   // w_{nx-1} = 0
      }
      global_sync();

      // ======== wave phase: B, G of the pass; Q = orth(W) for the next one ========
      const bool last = pass == A.K - 1;
      for (int t = 0; t < nlive; ++t) {
        double* X = slot0 + (size_t)t * (size_t)A.slot + tsz;
        const double* Tq = X + (size_t)(pass & 1) * xsz;
        double* Tw = X + (size_t)((pass + 1) & 1) * xsz;
        int fl = rayleigh_ritz<PC>(Tq, Tw, E, red, lane);
        if (last) {
          const int64_t st = grp * TPW + t;
          const int64_t bt = A.lanes[st];
          const bool unsolved = A.st[bt] != 0 || A.badin[st] != 0;
          const double nan = __builtin_nan("");
#pragma unroll
          for (int a = 0; a < 2 * PC * PC; a += 64) {
            const int el = (a + lane) % (PC * PC), ra = el / PC, rb = el - ra * PC;
            double* row = a + lane < PC * PC ? A.ritz : A.gram;
            if (row && ra < msub && rb < msub) row[((size_t)st * msub + ra) * msub + rb] = unsolved ? nan : red[a + lane];
          }
          if (A.basis) {
            for (int e = lane; e < E; e += 64) {
              const int i = e / NB, r = e - i * NB;
              double v[PC];
              load_entry<PC>(Tq, e, v);
#pragma unroll
              for (int j = 0; j < PC; ++j)
                if (j < msub) A.basis[(((size_t)st * msub + j) * NB + r) * nx + i] = unsolved ? nan : v[j];
            }
          }
        } else {
          fl |= orth<PC>(Tw, E, msub, red, lane);
        }
        pnp::lds_sync();   // red is free for the next system
        if (lane == 0) wflag[t] |= fl;
      }
      global_sync();
    }

    // ---- status of the system: any lane of the team, and what the wave phase saw ----
    pnp::lds_sync();
    ring[0][base + r0] = bad ? 1.0 : 0.0;
    pnp::lds_sync();
    const double anybad = team_sum<NB>(ring[0], ln);
    if (live && isP) {
      const bool unsolved = A.st[b] != 0 || A.badin[sys] != 0;
      const int wf = wflag[team];
      A.flags[sys] = unsolved ? 2 : ((anybad != 0.0 || (wf & 1)) ? 1 : ((wf & 2) ? 3 : 0));
    }
    pnp::lds_sync();   // the ring, the exchange buffers and the flags are free for the next group
  }
}

template <int NB>
static hipError_t launch(const KArgs& a, int64_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((modes_kernel<NB, CATMODES_MAX_SUBSPACE>), dim3((int)blocks), dim3(64), 0, st, a);
  return hipSuccess;
}

template <int NB>
static hipError_t resident(int* per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, modes_kernel<NB, CATMODES_MAX_SUBSPACE>, 64, 0);
}

}  // namespace catmodes

static_assert(CATMODES_OK == pnp::post::OK && CATMODES_EINVAL == pnp::post::ERR_INVAL && CATMODES_ENOMEM == pnp::post::ERR_NOMEM &&
                  CATMODES_EDEVICE == pnp::post::ERR_DEVICE && CATMODES_MAX_NX == pnp::post::MAX_NX && CATMODES_MAX_SPECIES == pnp::post::MAX_SPECIES,
              "catint_modes.h and pnp_post.h disagree");
static_assert(CATMODES_WALL_DIRICHLET == pnp::team::WALL_DIRICHLET && CATMODES_WALL_STERN == pnp::team::WALL_STERN &&
                  CATMODES_PIVOT_GROWTH_LIMIT == pnp::team::PIVOT_GROWTH_LIMIT,
              "catint_modes.h and pnp_team.h disagree");

struct catmodes_ctx : pnp::post::Ctx {};

extern "C" {

int catmodes_create(int32_t device, catmodes_ctx** out) { return pnp::post::create("catmodes_create", device, out); }
void catmodes_destroy(catmodes_ctx* ctx) { pnp::post::destroy(ctx); }
const char* catmodes_last_error(const catmodes_ctx* ctx) { return pnp::post::last_error(ctx); }
const char* catmodes_last_kernel(const catmodes_ctx* ctx) { return pnp::post::last_kernel(ctx); }
float catmodes_last_kernel_ms(const catmodes_ctx* ctx) { return pnp::post::last_kernel_ms(ctx); }

int catmodes_solve(catmodes_ctx* ctx, const pnp_device_view* view, const catmodes_params* p, const catmodes_outputs* out) {
  using namespace catmodes;
  static const char entry[] = "catmodes_solve";
  constexpr int PC = CATMODES_MAX_SUBSPACE;
  if (const int rc = check_view(ctx, entry, "catmodes_params", view, p, out)) return rc;
  if (out->struct_size != (int32_t)sizeof(catmodes_outputs))
    return fail(ctx, CATMODES_EINVAL, "catmodes_solve: catmodes_outputs.struct_size does not match this library");
  const int N = view->nspecies, nx = view->nx, NB = N + 1;
  const int64_t B = view->batch;
  char msg[256];
  if (const int rc = check_medium(ctx, entry, view, p)) return rc;
  if (const int rc = check_species(ctx, entry, p, N)) return rc;
  const int R = p->nreactions, W = p->n_wall, m = p->subspace, K = p->iterations;
  if (const int rc = check_nreactions(ctx, entry, R)) return rc;
  if (const int rc = check_nwall(ctx, entry, W)) return rc;
  if (const int rc = check_reactions(ctx, entry, p, N)) return rc;
  if (const int rc = check_wall(ctx, entry, p, N)) return rc;
  if (!p->phiM) return fail(ctx, CATMODES_EINVAL, "catmodes_solve: phiM is required");
  if (m < 1 || m > CATMODES_MAX_SUBSPACE) {
    snprintf(msg, sizeof msg, "catmodes_solve: subspace = %d outside [1, %d]", m, CATMODES_MAX_SUBSPACE);
    return fail(ctx, CATMODES_EINVAL, msg);
  }
  if (m > N * (nx - 1)) {
    snprintf(msg, sizeof msg, "catmodes_solve: subspace = %d above the rank of S, N (nx - 1) = %d", m, N * (nx - 1));
    return fail(ctx, CATMODES_EINVAL, msg);
  }
  if (K < 1 || K > CATMODES_MAX_ITERATIONS) {
    snprintf(msg, sizeof msg, "catmodes_solve: iterations = %d outside [1, %d]", K, CATMODES_MAX_ITERATIONS);
    return fail(ctx, CATMODES_EINVAL, msg);
  }
  if (const int rc = check_lanes(ctx, entry, p, B)) return rc;
  const int64_t n = p->nlanes;
  if (n > 0 && !p->start) return fail(ctx, CATMODES_EINVAL, "catmodes_solve: start is required");
  if (n == 0) return CATMODES_OK;

  KArgs a;
  memset(&a, 0, sizeof a);
  a.nx = nx; a.ldx = view->row_pitch; a.nreact = R; a.nwall = W; a.stern = p->wall_bc == CATMODES_WALL_STERN;
  a.m = m; a.K = K; a.nsys = n;
  a.c = view->c_dev; a.phi = view->phi_dev; a.st = view->status_dev;
  a.steric = fill_consts(a.k, p, N, a.stern);
  const int TPW = 64 / NB;
  const size_t nn = (size_t)n, E = (size_t)nx * NB, nstart = (size_t)m * E;
  a.slot = (int64_t)(even_(E * NB) + 2 * E * PC);

  // the inputs, staged on the host for one copy: edge weights, control volumes, row constants, potentials, rate constants, lanes (int64
  // in the place of doubles), the flags of non-finite inputs (int32 pairs), the start vectors, tables
  Inputs in;
  const int i_grid = declare_grid(in, a, nx), i_p = in.add((size_t)B, &a.phiM), i_k = in.add((size_t)B * W, &a.kwall),
            i_l = in.add_unpadded(nn, &a.lanes), i_b = in.add((nn + 1) / 2, &a.badin), i_s = in.add(nstart, &a.start),
            i_t = in.add_unpadded(sizeof(Table) / 8, &a.tab);
  const size_t n_in = in.total;
  try {
    ctx->stage.assign(n_in, 0.0);
    ctx->flags.assign(nn, 0);
  } catch (const std::bad_alloc&) {
    return fail(ctx, CATMODES_ENOMEM, "catmodes_solve: out of host memory");
  }
  stage_grid(in, ctx->stage, i_grid, p, nx, N);
  memcpy(in.host(ctx->stage, i_p), p->phiM, (size_t)B * 8);
  if (W) memcpy(in.host(ctx->stage, i_k), p->k, (size_t)B * W * 8);
  stage_lanes(in.host(ctx->stage, i_l), p);
  memcpy(in.host(ctx->stage, i_s), p->start, nstart * 8);
  {
    bool start_fin = true;
    for (size_t i = 0; i < nstart; ++i) start_fin = start_fin && std::isfinite(p->start[i]);
    int32_t* bi = reinterpret_cast<int32_t*>(in.host(ctx->stage, i_b));
    for (size_t i = 0; i < nn; ++i) {
      const int64_t b = p->lanes ? p->lanes[i] : (int64_t)i;
      bool fin = start_fin && std::isfinite(p->phiM[b]);
      for (int r = 0; r < W; ++r) fin = fin && std::isfinite(p->k[b * W + r]);
      bi[i] = fin ? 0 : 1;
    }
  }
  Table* tb = reinterpret_cast<Table*>(in.host(ctx->stage, i_t));
  fill_reactions(tb, p);
  fill_wall(tb, p, N);

  // the rows that were asked for
  const Row rows[] = {{out->ritz, &a.ritz, nn * m * m}, {out->gram, &a.gram, nn * m * m}, {out->basis, &a.basis, nn * m * E}};
  const size_t need_out = rows_doubles(rows), n_flags = even((nn + 1) / 2);
  if (!need_out && !out->status) return CATMODES_OK;

  PNP_POST_HIP(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)view->stream;
  // persistent grid: as many waves as the device holds at once unless the caller sizes it, no more than there are groups of systems
  // and no more than the workspace cap admits (at least one)
  const int64_t groups = ((int64_t)n + TPW - 1) / TPW;
  int64_t blocks = 0;
  if (const int rc = persistent_waves(ctx, entry, p->max_waves, [&](int* per_cu) {
        return dispatch_nb(NB, [&](auto nb) { return resident<decltype(nb)::value>(per_cu); });
      }, groups, &blocks))
    return rc;
  size_t cap = (size_t)2 << 30;
  if (const char* e = getenv("CATMODES_WORKSPACE_BYTES")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end && end != e && *end == 0) cap = (size_t)v;
  }
  const size_t per_wave = (size_t)TPW * (size_t)a.slot;   // doubles
  blocks = std::min<int64_t>(blocks, std::max<int64_t>(1, (int64_t)(cap / 8 / per_wave)));
  const size_t ws_doubles = (size_t)blocks * per_wave;
  const size_t ws_at = even(n_in + need_out + n_flags);   // the slots are read and written 16 bytes at a time
  if (const int rc = reserve(ctx, entry, ws_at + ws_doubles)) return rc;
  in.place(ctx->buf);
  a.flags = reinterpret_cast<int32_t*>(place_rows(rows, ctx->buf + n_in));
  a.ws = ctx->buf + ws_at;
  if (const int rc = run_with_status(ctx, entry, st, n_in, rows, out->status, a.flags, nn, [&] {
        return dispatch_nb(NB, [&](auto nb) { return launch<decltype(nb)::value>(a, blocks, st); });
      }))
    return rc;
  snprintf(msg, sizeof msg, "catmodes::modes_kernel<%d, %d>", NB, PC);
  ctx->last_kernel = msg;
  return CATMODES_OK;
}

}  // extern "C"
