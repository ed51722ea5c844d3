// The column-lane Newton kernels of the physical mode: the lane kernel of pnp_lane.hip with every block row shared by W lanes, W = 2
// (lane pair, pnp_lane2.hip) or 4 (lane quad, pnp_lane4.hip).  An operating point holds 2 W lanes -- two sweep directions x W column
// lanes -- and a wave 64 / (2 W) points.  This header is the scheme, written once: lane geometry, the cross-lane exchanges, the kernel
// body and the launcher; the two source files keep the kernels' names, the reasons each width exists and its batch window.
//   * the augmented block [D' | Ah | r] is distributed by COLUMNS: unknown j belongs to column lane j % W (local index j / W); the
//     right-hand side is column N+1 of [Ah | r].  D' column j = D column j - Bk T[:, j] needs only T's column j -- which the same lane
//     produced in the previous row -- so the elimination is formed without any exchange;
//   * Gauss-Jordan over the distributed columns: at pivot k the owner's column k reaches the other column lanes of its direction by one
//     DPP quad_perm broadcast per 32-bit half (no LDS, no select), all of them compute the same multipliers and update their own columns;
//   * species assembly is split: column lane q evaluates the edge fluxes of the species k with k % W == q, the others get them by DPP;
//   * the back-substitution sums each lane's partial products over its columns across the column lanes; the update pass splits the
//     ROWS between them.
// Same mathematics, damping, stopping rule, batch-innermost 16-byte layouts and software pipelining as pnp_lane.hip (the solve the
// reference hands to COMSOL, catint/comsol_model.py:465-516); MODE 0 point ions, 1 steric ions, 2 + homogeneous reactions
// (comsol_model.py:781-867) and the constant convection term (:901-903).  gfx950 / MI355X only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "pnp_lane_common.h"

namespace pnp {
namespace lane {

// ---- lane geometry: lane = 2 W * point + W * direction + column lane ------------------------------------------------------------------------
template <int W>
struct ColLanes {
  static_assert(W == 2 || W == 4, "a point's 2 W lanes exchange by quad_perm: W column lanes fill half a quad or a whole one");
  static constexpr int PG = 64 / (2 * W);                                             // operating points per wave
  __device__ static int point(int lane) { return lane / (2 * W); }
  __device__ static int col(int lane) { return lane & (W - 1); }                      // column lane: owns the columns j with j % W == col
  __device__ static bool down(int lane) { return (lane & W) != 0; }                   // false: from the wall upwards; true: from the bulk downwards
  // local columns of the augmented block [Ah | r] (NB + 1 columns) and of D' (NB columns); record doubles per lane and row (slots of
  // columns that do not exist stay untouched) and the same in 16-byte pairs
  static constexpr int cl(int nb) { return (nb + W) / W; }
  static constexpr int cld(int nb) { return (nb + W - 1) / W; }
  static constexpr int nrec(int nb) { return cl(nb) * nb; }
  static constexpr int rp(int nb) { return (nrec(nb) + 1) / 2; }
  // workspace per group of PG operating points: the records of a row (W column lanes) and the state, solution and two time levels
  static size_t rec_doubles(int nb, int nx) { return (size_t)nx * W * (size_t)(rp(nb) * 2) * PG; }
  static size_t state_doubles(int nb, int nx) { return (size_t)nx * (size_t)(2 * ((nb + 1) / 2 * 2) + 2 * (nb / 2 * 2)) * PG; }
};

// ---- the exchanges: every one stays inside a point's 2 W lanes ----------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double quad_perm(double v) {      // lane i of a quad reads lane (CTRL >> 2 i) & 3 of it
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, true);      // (mov_dpp: no "old" operand to materialise -- every lane of a quad is a valid source)
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
constexpr int QP_XOR1 = 1 | (0 << 2) | (3 << 4) | (2 << 6);
constexpr int QP_XOR2 = 2 | (3 << 2) | (0 << 4) | (1 << 6);
// the value of column lane Q of the own direction, in all its column lanes (W = 2: a quad holds both directions of a point)
template <int W, int Q>
__device__ __forceinline__ double col_bcast(double v) {
  static_assert(Q >= 0 && Q < W, "no such column lane");
  if constexpr (W == 4) return quad_perm<Q | (Q << 2) | (Q << 4) | (Q << 6)>(v);
  else return quad_perm<Q | (Q << 2) | ((2 + Q) << 4) | ((2 + Q) << 6)>(v);
}
// (Q known after unrolling: the chain folds to one broadcast)
template <int W>
__device__ __forceinline__ double col_bcast_sel(const int Q, double v) {
  if constexpr (W == 4) return Q == 0 ? col_bcast<4, 0>(v) : (Q == 1 ? col_bcast<4, 1>(v) : (Q == 2 ? col_bcast<4, 2>(v) : col_bcast<4, 3>(v)));
  else return Q == 0 ? col_bcast<2, 0>(v) : col_bcast<2, 1>(v);
}
// the same column lane of the other direction
template <int W>
__device__ __forceinline__ double other_dir(double v) {
  if constexpr (W == 4) return __shfl_xor(v, 4, 64);
  else return quad_perm<QP_XOR2>(v);
}
// sum and maximum over the column lanes of a direction, in all of them
template <int W>
__device__ __forceinline__ double col_sum(double v) {
  v += quad_perm<QP_XOR1>(v);
  if constexpr (W == 4) v += quad_perm<QP_XOR2>(v);
  return v;
}
template <int W>
__device__ __forceinline__ double col_max(double v) {
  v = fmax(v, quad_perm<QP_XOR1>(v));
  if constexpr (W == 4) v = fmax(v, quad_perm<QP_XOR2>(v));
  return v;
}
// element W jj + q of a table of LEN entries (0 beyond its end): compile-time indices, the column lane q selects
template <int W, typename Tab>
__device__ __forceinline__ double pickq(Tab&& tab, const int q, const int jj, const int LEN) {
  double v = 0.0;
#pragma unroll
  for (int Q = 0; Q < W; ++Q)
    if (W * jj + Q < LEN) v = (q == Q) ? tab(W * jj + Q) : v;
  return v;
}

// ---- where the two widths differ on purpose -----------------------------------------------------------------------------------------------------------
// Rows requested ahead in the back-substitution (records) and in the update pass (solution and state), into a ring of that many
// register buffers.  Lane quad: a row of the back-substitution is a few hundred instructions against 14 record loads, and one row
// ahead the pass ran at one memory round trip per row (34 % of the wave's life in s_waitcnt at one wave per SIMD); four rows ahead
// removed that.  Lane pair: a lane's record is twice as long (NB = 9: 23 pairs, 92 registers per ring slot) and its NB = 9 instances
// spill already with one slot (profiles/lane_cols.md), so it keeps one.  Depth 1 is the plain one-row-ahead prefetch.
template <int W> constexpr int PREFETCH_ROWS = W == 4 ? 4 : 1;
// Start stagger (NewtonArgs::lane_stagger, option LANE_STAGGER), lane quad only: every wave of a launch starts with a forward pass
// (writes, ~75 % of an iteration) followed by a back-substitution that reads its records back at several TB/s -- with one wave per SIMD
// and equal row times the whole chip is in the same pass at the same time, the back-substitutions of all 1024 waves hit HBM together
// (5 TB/s, 2.7 x the cycles per row of a wave alone on the chip) and the forward passes leave it idle.  Four groups of waves start a
// quarter of an iteration apart (tools/probe/lane4_stagger.sh).  The lane pair never had it: the option is the quad's, and nothing
// has been measured for the pair.
template <int W> constexpr bool START_STAGGER = W == 4;

// The update pass clips a row either through newton_clip_row (pnp_math.h) after the loop that takes the update norm, or with the same
// scalar functions inside that loop.  Measured (profiles/newton_rule.md section 5, 8 x 512 x 8192 points, parent and forms alternating): the
// lane pair is 1.0 to 1.5 % behind its hand-written predecessor with the first form and level (+0.3 ... +0.5 %) with the second; the
// lane quad is 0.8 % behind with the first and 1.5 to 1.9 % with the second.  Each keeps the form that is faster for it.
template <int W> constexpr bool CLIPS_WITH_THE_NORM = W == 2;

// ---- the kernel body --------------------------------------------------------------------------------------------------------------------------------------
// (BDF: the BDF2 history inside the launch -- a template flag here: as a run-time flag it cost the backward-Euler instances 3-8 % in
// registers moved around, tools/probe/ab_old_new.sh)
template <int W, int NB, int MODE, bool BDF>
__device__ __forceinline__ void newton_lane_cols_body(const NewtonArgs& G) {
  using LC = ColLanes<W>;
  constexpr int N = NB - 1;
  constexpr int PG = LC::PG;
  constexpr int CL = LC::cl(NB), CLD = LC::cld(NB), RP = LC::rp(NB);
  constexpr int VP = (NB + 1) / 2, CP = (N + 1) / 2;
  constexpr bool MPB = MODE >= 1;
  constexpr bool FULL = MODE == 2;
  __shared__ double s_cb[N][PG];
  __shared__ LaneParams sP;
  // MODE 2 only (no LDS in the other instances): the flattened mass-action table and the per-row values its slots point into
  __shared__ double s_react[FULL ? sizeof(ReactionSides) / sizeof(double) + RC_ROWS * 64 : 1];
  ReactionSides& sS = *(ReactionSides*)s_react;
  double (*s_rc)[64] = (double (*)[64])(s_react + sizeof(ReactionSides) / sizeof(double));
  const int lane = threadIdx.x, o = LC::point(lane);
  const int q = LC::col(lane);
  const bool side = LC::down(lane);
  const double sgn = side ? -1.0 : 1.0;
  const int nx = G.nx;
  const int m = (nx - 1) >> 1;
  const int n_dn = nx - 2 - m;
  const int64_t g = blockIdx.x;
  const int64_t slot = (G.lane_group0 + g) * PG + o;
  const int64_t slot_c = slot < G.B ? slot : G.B - 1;
  const int64_t b = G.lane_perm ? (int64_t)G.lane_perm[slot_c] : slot_c;      // the operating point these 2 W lanes hold
  const bool valid = slot < G.B && !(G.lane_mask && !G.lane_mask[b]);
  d2* ts = (d2*)G.lane_ts + (size_t)g * (size_t)nx * VP * PG + o;
  d2* xs = (d2*)G.lane_xs + (size_t)g * (size_t)nx * VP * PG + o;
  d2* tco = (d2*)G.lane_tco + (size_t)g * (size_t)nx * CP * PG + o;
  d2* tcn = (d2*)G.lane_tcn + (size_t)g * (size_t)nx * CP * PG + o;      // BDF2: the time level before the previous one
  d2* rec = (d2*)G.lane_rec + (size_t)g * (size_t)nx * W * RP * PG + (size_t)q * RP * PG + o;      // this column lane's records
  auto TS = [&](int i, int p) -> d2& { return ts[((size_t)i * VP + p) * PG]; };
  auto XS = [&](int i, int p) -> d2& { return xs[((size_t)i * VP + p) * PG]; };
  auto CO = [&](int i, int p) -> d2& { return tco[((size_t)i * CP + p) * PG]; };
  auto CN = [&](int i, int p) -> d2& { return tcn[((size_t)i * CP + p) * PG]; };
  auto REC = [&](int i, int p) -> d2& { return rec[((size_t)i * W * RP + p) * PG]; };
  const double phiM = G.pb[b * 4 + 0], phiB = G.pb[b * 4 + 1];
  if ((lane & (2 * W - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) s_cb[k][o] = G.cbulk[(size_t)b * N + k];
  }
  if (lane < PNP_NEWTON_MAX_SPECIES) {
    sP.sig[lane] = G.sig[lane];
    sP.peq[lane] = G.peq[lane];
    sP.pe[lane] = G.pe[lane];
    sP.rs[lane] = G.rs[lane];
    sP.qb[lane] = G.qb[lane];
  }
  if constexpr (FULL) {
    lane_stage_reaction_sides(sS, G.sides, lane);
    lane_reaction_init(s_rc, lane);
  }
  __syncthreads();
  auto fwd_row = [&](int s) { return side ? (s < n_dn ? nx - 2 - s : m + 1) : (s < m ? s : m); };
  auto col_j = [&](const int jj) { return W * jj + q; };      // unknown of local column jj (run-time lane, compile-time jj)
  auto pick = [&](auto&& tab, const int jj, const int LEN) { return pickq<W>(tab, q, jj, LEN); };
  // pairs of this lane's record that hold columns which exist (column j = W jj + q <= NB): the others are never stored nor loaded
  const int ncol = (NB - q) / W + 1;                        // local columns with j <= NB
  const int rp_valid = (ncol * NB + 1) / 2;

  bool have = valid, fresh = true;
  int step = 0, it = 0, total_it = 0, st = PNP_STATUS_OK;
  double upd_prev = INFINITY;
  double alarm = 0.0;            // pivot monitor (sticky)
  if constexpr (START_STAGGER<W>)
    for (int z = (int)(g & 3) * G.lane_stagger; z > 0; --z) __builtin_amdgcn_s_sleep(127);
#ifdef PNP_LANE_STAMPS
  double stamp_f = 0.0, stamp_b = 0.0, stamp_u = 0.0, stamp_n = 0.0;
  double row_a = 0.0, row_d = 0.0, row_g = 0.0, row_s = 0.0, row_n = 0.0;      // forward row: assembly / D' and Ah columns / Gauss-Jordan / stores
#endif

  for (;;) {
    if (__ballot(have) == 0ull) break;
#ifdef PNP_LANE_STAMPS
    const unsigned long long ts0 = __builtin_readcyclecounter();
#endif
    const NewtonArgs& A = G;
    // first iteration of a timestep: the previous time level is the state itself -- unless the caller prepared it (BDF2: G.ext_old)
    const bool first = fresh && !G.ext_old;
    // BDF2 inside a launch of several timesteps (G.bdf2, lane kernels): a step has a history -- the time level before the previous one,
    // kept in CN -- if the launch started with one or it is not the operating point's first step; then the previous-level value is the
    // combination (4 c_n - c_n-1) / 3 and 1/dt carries 3/2 (pnp_capi.hip: newton_timesteps; comsol_model.py:518-531, maxorder 2)
    const bool hist = BDF && have && (G.bdf_hist0 || step > 0);
    const double sgs = (BDF && hist) ? 1.5 : 1.0;
    if (fresh) {
      it = 0;
      upd_prev = INFINITY;
      fresh = false;
    }
    it += 1;
    // =========================== forward ===================================================================================
    int poff = 0;
    asm volatile("" : "+v"(poff));
    const LaneParams* P = (const LaneParams*)((const char*)&sP + poff);
    double hc[N], hphi, hw = 0.0, hinv = 1.0;
    double bphi = 0.0, binv = 1.0;
    double eJ[N], eBd[N], eBn[N], eJu[N];                 // behind edge, every species, in all column lanes
    // this lane's columns of the behind record [T | t], [row][local column]: the SAME registers hold the augmented block [Ah | r] of the
    // row being eliminated -- column jj of the new block depends on column jj of the record only, so it is built in place and what
    // the Gauss-Jordan leaves there is the next row's record (no copy at the end of a row, 54 registers less to keep alive)
    double Xl[NB][CL];
#pragma unroll
    for (int jj = 0; jj < CL; ++jj)
#pragma unroll
      for (int r = 0; r < NB; ++r) Xl[r][jj] = 0.0;
    d2 p_a[VP], p_co[CP];
    // (first iteration of a BDF2 step with a history: the previous-level slot of the prefetch carries the level BEFORE the previous one
    //  -- the previous level of such an iteration is formed from the state itself and not read; one pointer chosen per iteration)
    const d2* tprev = (BDF && first && hist) ? tcn : tco;
    double p_vi, p_wea, p_web;
    auto request = [&](int s) {
#ifdef L4_NO_REQUEST      // (diagnosis build: every row reads the first one again -- cache hits)
      const int i = fwd_row(0) + 0 * s;
#else
      const int i = fwd_row(s);
#endif
      const int ia = side ? i - 1 : i + 1;
#pragma unroll
      for (int p = 0; p < VP; ++p) p_a[p] = TS(ia, p);
#pragma unroll
      for (int p = 0; p < CP; ++p) p_co[p] = tprev[((size_t)i * CP + p) * PG];
      p_vi = G.gv[i];
      p_wea = G.gw[side ? i - 1 : i];
      p_web = G.gw[side ? i : (i > 0 ? i - 1 : 0)];
    };
    double mphi = 0.0;
    {
      const int i = side ? nx - 2 : 0;
      d2 h2[VP], b2[VP];
#pragma unroll
      for (int p = 0; p < VP; ++p) {
        h2[p] = TS(i, p);
        b2[p] = TS(nx - 1, p);
      }
      request(0);
#pragma unroll
      for (int k = 0; k < N; ++k) {
        hc[k] = h2[k >> 1][k & 1];
        eJ[k] = 0.0;
        eBd[k] = 0.0;
        eBn[k] = 0.0;
        eJu[k] = 0.0;
      }
      hphi = h2[N >> 1][N & 1];
      if constexpr (MPB) {
        double f = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) f = __builtin_fma(G.vol[k], hc[k], f);
        hw = -log1p_sc(-f);
        hinv = 1.0 / (1.0 - f);
      }
      if (side) {        // the bulk row is the downward direction's initial state (see pnp_lane.hip); all its column lanes evaluate it alike
        double bc[N], bw = 0.0, tb[NB];
#pragma unroll
        for (int k = 0; k < N; ++k) bc[k] = b2[k >> 1][k & 1];
        bphi = b2[N >> 1][N & 1];
        if constexpr (MPB) {
          double f = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) f = __builtin_fma(G.vol[k], bc[k], f);
          bw = -log1p_sc(-f);
          binv = 1.0 / (1.0 - f);
        }
        const double we = G.gw[nx - 2];
        const double dphi = bphi - hphi, dw = bw - hw;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const LEdge e = lane_edge_flux(__builtin_fma(G.qb[k], dphi, dw) - (FULL ? sP.pe[k] / we : 0.0), hc[k], bc[k], we);
          eJ[k] = e.J;
          eBd[k] = e.Bp;
          eBn[k] = e.Bm;
          eJu[k] = e.Ju;
          tb[k] = -(bc[k] - s_cb[k][o]);
        }
        tb[N] = -(bphi - phiB);
        mphi = newton_norm_phi(0.0, tb[N]);
        // t is column NB of [T | t]: it lives in column lane NB % W, local index NB / W
        if (q == NB % W) {
#pragma unroll
          for (int r = 0; r < NB; ++r) Xl[r][NB / W] = tb[r];
        }
        if (q == 0) {
#pragma unroll
          for (int p = 0; p < VP; ++p) {
            d2 v;
            v[0] = tb[2 * p];
            v[1] = 2 * p + 1 < NB ? tb[2 * p + 1 < NB ? 2 * p + 1 : 0] : 0.0;
            XS(nx - 1, p) = v;
          }
          if (first) {
#pragma unroll
            for (int p = 0; p < CP; ++p) {
              d2 v;
              v[0] = bc[2 * p];
              v[1] = 2 * p + 1 < N ? bc[2 * p + 1 < N ? 2 * p + 1 : 0] : 0.0;
              CO(nx - 1, p) = v;
              if (BDF && have) CN(nx - 1, p) = v;
            }
          }
        }
      }
    }
    const int S = (n_dn > m ? n_dn : m) + 1;
    for (int s = 0; s < S; ++s) {
      const bool last = s == S - 1;
      const bool act = last ? !side : (side ? s < n_dn : s < m);
      double ac[N], aphi, co[N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        ac[k] = p_a[k >> 1][k & 1];
        co[k] = p_co[k >> 1][k & 1];
      }
      aphi = p_a[N >> 1][N & 1];
      const double vi = p_vi, wea = p_wea, web = p_web;
      if (!last) request(s + 1);
      if (last) {       // the middle row reads the downward direction's last record back from device memory (see pnp_lane.hip)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_wave_barrier();
      }
      if (act) {
#ifdef PNP_LANE_STAMPS
        const unsigned long long r0 = __builtin_readcyclecounter();
#endif
        asm volatile("" : "+v"(poff));
        P = (const LaneParams*)((const char*)&sP + poff);
        const int i = fwd_row(s);
        const bool wall = s == 0 && !side;
        double aw = 0.0, ainv = 1.0;
        if constexpr (MPB) {
          double f = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) f = __builtin_fma(G.vol[k], ac[k], f);
          aw = -log1p_sc(-f);
          ainv = 1.0 / (1.0 - f);
        }
        // ---- ahead edge: column lane q evaluates the species k with k % W == q, the other column lanes get them by broadcast -------------
        double aJ[N], aBd[N], aBn[N], aJu[N];
        {
          const double dphi = aphi - hphi, dw = aw - hw;
          const double rwea = FULL ? 1.0 / wea : 0.0;
#pragma unroll
          for (int kk = 0; kk < (N + W - 1) / W; ++kk) {
            // (a group with fewer than W species: the spare lanes recompute its last one)
            auto clampk = [&](int k) { return k < N ? k : N - 1; };
            const int kq = clampk(W * kk + q);          // this lane's species of the group
            const double qb_ = P->qb[kq];
            double hc_ = hc[clampk(W * kk)], ac_ = ac[clampk(W * kk)];
#pragma unroll
            for (int Q = 1; Q < W; ++Q) {
              hc_ = q == Q ? hc[clampk(W * kk + Q)] : hc_;
              ac_ = q == Q ? ac[clampk(W * kk + Q)] : ac_;
            }
            double pe_ = 0.0;
            if constexpr (FULL) pe_ = P->pe[kq];
            const double u = sgn * __builtin_fma(qb_, dphi, dw) - (FULL ? pe_ * rwea : 0.0);
            const double cl = side ? ac_ : hc_, cr = side ? hc_ : ac_;
#ifdef L4_CHEAP_EDGE      // (diagnosis build: the edge without its exponential)
            LEdge e;
            e.Bp = wea * (1.0 - 0.5 * u);
            e.Bm = wea * (1.0 + 0.5 * u);
            e.J = -(e.Bm * cr - e.Bp * cl);
            e.Ju = -wea * 0.5 * (cr + cl);
#else
            const LEdge e = lane_edge_flux(u, cl, cr, wea);
#endif
            const double mJ = sgn * e.J, mBd = side ? e.Bm : e.Bp, mBn = side ? e.Bp : e.Bm, mJu = e.Ju;
#pragma unroll
            for (int Q = 0; Q < W; ++Q) {
              const int k = W * kk + Q;
              if (k < N) {
                aJ[k] = col_bcast_sel<W>(Q, mJ);
                aBd[k] = col_bcast_sel<W>(Q, mBd);
                aBn[k] = col_bcast_sel<W>(Q, mBn);
                aJu[k] = col_bcast_sel<W>(Q, mJu);
              }
            }
          }
        }
        // ---- right-hand side and the diagonal block's ingredients (every species, all column lanes) -----------------------------------
        double rhs[NB], diag[N], Js[N];
        double rho = 0.0;
        double cs_[N];      // the previous-level value of this step: the state itself (backward Euler) or the BDF2 combination
#pragma unroll
        for (int k = 0; k < N; ++k) cs_[k] = hc[k];
        if (BDF && first && hist) {      // (under its own branch: eight divisions that only the first iteration of a BDF2 step needs)
#pragma unroll
          for (int k = 0; k < N; ++k) cs_[k] = (4.0 * hc[k] - co[k]) / 3.0;
        }
        if (first && q == 0) {
#pragma unroll
          for (int p = 0; p < CP; ++p) {
            d2 v;
            v[0] = cs_[2 * p];
            v[1] = 2 * p + 1 < N ? cs_[2 * p + 1 < N ? 2 * p + 1 : 0] : 0.0;
            CO(i, p) = v;
            if (BDF && have) {      // (a finished point runs along with its wave: its history stays)
              d2 w_;
              w_[0] = hc[2 * p];
              w_[1] = 2 * p + 1 < N ? hc[2 * p + 1 < N ? 2 * p + 1 : 0] : 0.0;
              CN(i, p) = w_;
            }
          }
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double cok = first ? cs_[k] : co[k];
          const double sg = vi * P->sig[k] * sgs;
          rho = __builtin_fma(P->peq[k], hc[k], rho);
          double F = sg * (hc[k] - cok) + aJ[k] + eJ[k];
          if (wall) F -= G.flux[(size_t)b * N + k] * A.fl[k];
          rhs[k] = -F;
          diag[k] = sg + aBd[k] + eBd[k];
          Js[k] = aJu[k] + eJu[k];
        }
        double dNN, ahNN;
        if (wall) {
          if (A.wall_bc == 0) {
            rhs[N] = -(hphi - phiM);
            dNN = 1.0;
            ahNN = 0.0;
          } else {
            rhs[N] = -(wea * (aphi - hphi) + A.stern * (phiM - A.phi_pzc - hphi));
            dNN = -wea - A.stern;
            ahNN = wea;
          }
        } else {
          rhs[N] = -((wea * (aphi - hphi) + web * (bphi - hphi)) + vi * rho);
          dNN = -(wea + web);
          ahNN = wea;
        }
        const double pq = wall ? 0.0 : vi;
#ifdef PNP_LANE_STAMPS
        // (the stamps of a row must wait for the section's results: the counter read is scalar code the scheduler would float over the
        //  vector work -- a sum of everything the section produced is handed to an empty asm first)
        {
          double z = rhs[N] + dNN;
#pragma unroll
          for (int k = 0; k < N; ++k) z += (rhs[k] + diag[k]) + (Js[k] + aBn[k]);
          asm volatile("" ::"v"(z));
        }
        const unsigned long long r1 = __builtin_readcyclecounter();
#endif
        // ---- this lane's columns of D' = D - Bk T and of [Ah | r - Bk t] ---------------------------------------------------------------
        double Dl[NB][CLD];           // [row][local column]
        // (Bk col)[k] = -eBn_k col[k] + eJu_k (qb_k col[N] + binv sum_q vol_q col[q]),  (Bk col)[N] = web col[N]
        auto minus_bk = [&](const double (&col)[NB], double (&v)[NB], const double (&bn)[N], const double (&ju)[N], double inv_, double wN) {
          double sj = 0.0;
          if constexpr (MPB) {
#pragma unroll
            for (int qq = 0; qq < N; ++qq) sj = __builtin_fma(G.vol[qq], col[qq], sj);
            sj *= inv_;
          }
#pragma unroll
          for (int k = 0; k < N; ++k) {
            v[k] = __builtin_fma(bn[k], col[k], v[k]);
            v[k] = __builtin_fma(-ju[k], __builtin_fma(G.qb[k], col[N], sj), v[k]);
          }
          v[N] = __builtin_fma(-wN, col[N], v[N]);
        };
#pragma unroll
        for (int jj = 0; jj < CL; ++jj) {
          const int j = col_j(jj);                      // (run-time column lane, compile-time jj)
          const bool isrhs = j == NB, isphi = j == N;
          double volj = 0.0;
          if constexpr (MPB) volj = pick([&](int k) { return G.vol[k]; }, jj, N);
          const double peqj = pick([&](int k) { return P->peq[k]; }, jj, N);
          double v[NB];
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const bool dk = (k / W) == jj && (k % W) == q;                            // k == j
            double d = MPB ? -Js[k] * (volj * hinv) : 0.0;                            // (volj = 0 outside the species columns)
            d = dk ? d + diag[k] : d;
            d = isphi ? -G.qb[k] * Js[k] : d;
            v[k] = isrhs ? rhs[k] : (j > NB ? 0.0 : d);
          }
          v[N] = isrhs ? rhs[N] : (isphi ? dNN : (j > NB ? 0.0 : pq * peqj));
          double col[NB];
#pragma unroll
          for (int r = 0; r < NB; ++r) col[r] = Xl[r][jj];
          minus_bk(col, v, eBn, eJu, binv, web);
          // D' has columns j < NB, the augmented block gets the right-hand side (j == NB) here and the Ah columns below
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            if (jj < CLD) Dl[r][jj < CLD ? jj : 0] = j >= NB ? 0.0 : v[r];
            Xl[r][jj] = v[r];            // (kept where j == NB; overwritten with the Ah column otherwise)
          }
        }
        // ---- implicit wall kinetics (see pnp_lane.hip / fill_row) -------------------------------------------------------------------------
        if (wall && A.n_wk > 0) {
          for (int w_ = 0; w_ < A.n_wk; ++w_) {
            const int sp = A.wk_species[w_];
            double cs = 1.0;
#pragma unroll
            for (int k = 0; k < N; ++k) cs = (k == sp) ? hc[k] : cs;
            const double kr = G.wk_k[(size_t)b * PNP_MAX_WALL_REACTIONS + w_];
            const double al = A.wk_alpha[w_], den = 1.0 / (1.0 + A.wk_sat[w_] * cs);
            const double E = al != 0.0 ? exp(al * (phiM - hphi)) : 1.0;
            const double gq = cs * den * E, dg = den * den * E;
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const double a = A.wk_nu[w_][k] * kr * A.fl[k];
#pragma unroll
              for (int jj = 0; jj < CL; ++jj) {
                const int j = col_j(jj);
                if (jj < CLD) {
                  if (j < N && j == sp) Dl[k][jj < CLD ? jj : 0] -= a * dg;
                  if (j == N && al != 0.0) Dl[k][jj < CLD ? jj : 0] += a * al * gq;
                }
                if (j == NB) Xl[k][jj] += a * gq;
              }
            }
          }
        }
        // ---- homogeneous reactions (see pnp_lane.hip): every lane evaluates the rates, each column lane keeps its own columns -----------------
        if constexpr (FULL) {
          const int ns = __builtin_amdgcn_readfirstlane(sS.n);
          if (ns > 0) {
            double vrs[N];
#pragma unroll
            for (int k = 0; k < N; ++k) vrs[k] = vi * P->rs[k];
            lane_reaction_fill<N>(s_rc, lane, hc, hinv);
            // (two sides per pass: their LDS round trips -- table entry, then the values it points at -- overlap)
            for (int sd = 0; sd < ns; sd += 2) {
              const ReactionSides::Side& Sa = sS.side[sd];
              const ReactionSides::Side& Sb = sS.side[sd + 1];
              const LaneSide ra = lane_reaction_side<MPB>(Sa, s_rc, lane);
              const LaneSide rb = lane_reaction_side<MPB>(Sb, s_rc, lane);
              double dla[CL], dlb[CL];           // d prod / d c_j of this lane's columns
#pragma unroll
              for (int jj = 0; jj < CL; ++jj) {
                double volj = 0.0;
                if constexpr (MPB) volj = pick([&](int k) { return G.vol[k]; }, jj, N);
                dla[jj] = col_j(jj) < N ? lane_side_dprod(ra, col_j(jj), volj) : 0.0;
                dlb[jj] = col_j(jj) < N ? lane_side_dprod(rb, col_j(jj), volj) : 0.0;
              }
#pragma unroll
              for (int k = 0; k < N; ++k) {
                const double wa = Sa.w[k] * vrs[k], wb = Sb.w[k] * vrs[k];
#pragma unroll
                for (int jj = 0; jj < CL; ++jj) {
                  if (jj < CLD) Dl[k][jj < CLD ? jj : 0] = __builtin_fma(-wb, dlb[jj], __builtin_fma(-wa, dla[jj], Dl[k][jj < CLD ? jj : 0]));
                  if (col_j(jj) == NB) Xl[k][jj] = __builtin_fma(wb, rb.prod, __builtin_fma(wa, ra.prod, Xl[k][jj]));
                }
              }
            }
          }
        }
        if (last) {
          // ---- middle row: the downward direction's record of row m+1 (same column lane, same local columns) enters with the ahead block ----
          const d2* other = (const d2*)G.lane_rec + (size_t)g * (size_t)nx * W * RP * PG + (size_t)q * RP * PG + o;
#pragma unroll
          for (int jj = 0; jj < CL; ++jj) {
            const int j = col_j(jj);
            const bool isrhs = j == NB;
            double col[NB], v[NB];
#pragma unroll
            for (int r = 0; r < NB; ++r) {
              const int e = jj * NB + r;
              double cv = 0.0;
              if (j <= NB)      // (columns that do not exist were never stored)
                cv = __hip_atomic_load((const double*)&other[((size_t)(m + 1) * W * RP + (e >> 1)) * PG] + (e & 1), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
              col[r] = cv;
              v[r] = isrhs ? Xl[r][jj] : (jj < CLD ? Dl[r][jj < CLD ? jj : 0] : 0.0);
            }
            minus_bk(col, v, aBn, aJu, ainv, ahNN);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
              if (jj < CLD) Dl[r][jj < CLD ? jj : 0] = j >= NB ? 0.0 : v[r];
              if (isrhs) Xl[r][jj] = v[r];
            }
          }
        }
        // ---- the Ah columns of the augmented block: Ah[k][j] = -aBn_k [j == k] + aJu_k (qb_k [j == N] + vol_j ainv), Ah[N][N] = ahNN ---------
#pragma unroll
        for (int jj = 0; jj < CL; ++jj) {
          const int j = col_j(jj);
          const bool isrhs = j == NB, isphi = j == N;
          double volj = 0.0;
          if constexpr (MPB) volj = pick([&](int k) { return G.vol[k]; }, jj, N);
#pragma unroll
          for (int k = 0; k < N; ++k) {
            const bool dk = (k / W) == jj && (k % W) == q;
            double y = MPB ? aJu[k] * (volj * ainv) : 0.0;
            y = dk ? y - aBn[k] : y;
            y = isphi ? aJu[k] * G.qb[k] : y;
            y = (j > NB || last) ? 0.0 : y;                 // (no such column: a spare slot; middle row: only the right-hand side)
            Xl[k][jj] = isrhs ? Xl[k][jj] : y;
          }
          Xl[N][jj] = isrhs ? Xl[N][jj] : ((isphi && !last) ? ahNN : 0.0);
        }
#ifdef PNP_LANE_STAMPS
        {
          double z = 0.0;
#pragma unroll
          for (int r = 0; r < NB; ++r) {
#pragma unroll
            for (int jj = 0; jj < CL; ++jj) z += Xl[r][jj] + (jj < CLD ? Dl[r][jj < CLD ? jj : 0] : 0.0);
          }
          asm volatile("" ::"v"(z));
        }
        const unsigned long long r2 = __builtin_readcyclecounter();
#endif
        // ---- Gauss-Jordan over the distributed columns ------------------------------------------------------------------------------------------
#ifdef L4_NO_GJ      // (diagnosis build, tools/probe/lane4_stamps.sh: what the row costs without its elimination; results are wrong)
#pragma unroll
        for (int k = 0; k < 0; ++k) {
#else
#pragma unroll
        for (int k = 0; k < NB; ++k) {
#endif
          double pc[NB];
#pragma unroll
          for (int r = 0; r < NB; ++r) pc[r] = col_bcast_sel<W>(k % W, Dl[r][k / W]);
          {   // pivot monitor (pnp_lane_common.h): rows k+1 .. of the pivot column against the pivot
            double cmax = 0.0;
#pragma unroll
            for (int r = k + 1; r < NB; ++r) cmax = fmax(cmax, fabs(pc[r]));
            alarm = (fabs(pc[k]) * G.lane_pivot_limit < cmax) ? 1.0 : alarm;
          }
          const double inv = nrcp(pc[k]);
#pragma unroll
          for (int jj = 0; jj < CLD; ++jj) {
            if (W * jj + W - 1 <= k) continue;          // columns j <= k are finished in all column lanes (the pivot column is not needed again)
            const double t_ = Dl[k][jj] * inv;
#pragma unroll
            for (int r = 0; r < NB; ++r) Dl[r][jj] = r == k ? t_ : __builtin_fma(-pc[r], t_, Dl[r][jj]);
          }
#pragma unroll
          for (int jj = 0; jj < CL; ++jj) {
            const double t_ = Xl[k][jj] * inv;
#pragma unroll
            for (int r = 0; r < NB; ++r) Xl[r][jj] = r == k ? t_ : __builtin_fma(-pc[r], t_, Xl[r][jj]);
          }
        }
#ifdef PNP_LANE_STAMPS
        {
          double z = 0.0;
#pragma unroll
          for (int r = 0; r < NB; ++r) {
#pragma unroll
            for (int jj = 0; jj < CL; ++jj) z += Xl[r][jj];
          }
          asm volatile("" ::"v"(z));
        }
        const unsigned long long r3 = __builtin_readcyclecounter();
#endif
        // The next row's inputs (requested at the top of this row) are made to ARRIVE here, before this row's record stores are issued:
        // vector memory operations retire in order and the compiler's wait-count bookkeeping is conservative across the loop's back
        // edge -- left to itself it consumes these loads after the stores with s_waitcnt vmcnt(0), i.e. every row waits for its own
        // record stores to reach memory (+4 k cycles per row at 1024 waves, tools/probe/lane4_stamps.sh with -DL4_NO_REC_STORE).
        // After a whole row of arithmetic the loads have long landed; the stores then drain behind the next row.  (A sum that needs
        // every loaded register, handed to an empty asm: values are only READ here -- redefining them under this
        // block's partial execution mask loses them for the resting lanes.)
        {
          double touch = (p_vi + p_wea) + p_web;
#pragma unroll
          for (int p = 0; p < VP; ++p) touch += p_a[p][0];
#pragma unroll
          for (int p = 0; p < CP; ++p) touch += p_co[p][0];
          asm volatile("" ::"v"(touch));
        }
        // ---- the record: this lane's columns, in 16-byte pairs (pairs of columns that do not exist are skipped) -----------------------------
        double held = 0.0;
#pragma unroll
        for (int jj = 0; jj < CL; ++jj)
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            const int e = jj * NB + r;
            if ((e & 1) == 0) {
              held = Xl[r][jj];
              if (e == CL * NB - 1) {
                d2 pr;
                pr[0] = held;
                pr[1] = 0.0;
#ifndef L4_NO_REC_STORE
                if ((e >> 1) < rp_valid) __builtin_nontemporal_store(pr, &REC(i, e >> 1));
#endif
              }
            } else {
              d2 pr;
              pr[0] = held;
              pr[1] = Xl[r][jj];
#ifndef L4_NO_REC_STORE      // (diagnosis builds, tools/probe/lane4_stamps.sh: results are wrong)
              if ((e >> 1) < rp_valid) __builtin_nontemporal_store(pr, &REC(i, e >> 1));
#else
              asm volatile("" :: "v"(pr));
#endif
            }
          }
        // (middle row: x_m = the solved right-hand side now sits in its owner's t slot Xl[.][NB / W], where the hand-over below takes it;
        //  the zero Ah columns of that row leave zeros in the other slots)
        bphi = hphi;
        binv = hinv;
        hphi = aphi;
        hw = aw;
        hinv = ainv;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          hc[k] = ac[k];
          eJ[k] = -aJ[k];
          eBn[k] = aBd[k];
          eBd[k] = aBn[k];
          eJu[k] = aJu[k];
        }
#ifdef PNP_LANE_STAMPS
        {
          const unsigned long long r4 = __builtin_readcyclecounter();
          row_a += (double)(r1 - r0);
          row_d += (double)(r2 - r1);
          row_g += (double)(r3 - r2);
          row_s += (double)(r4 - r3);
          row_n += 1.0;
        }
#endif
      }
    }
#ifdef PNP_LANE_STAMPS
    const unsigned long long ts1 = __builtin_readcyclecounter();
#endif
    // =========================== backward ========================================================================================================
    // x_m sits in the upward direction's column lane NB % W (local column NB / W); the upward direction broadcasts it, the downward
    // one takes it from its partner lanes
    double x[NB];
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      const double up = col_bcast<W, NB % W>(Xl[r][NB / W]);
      const double from_up = other_dir<W>(up);            // (cross-lane: every lane takes part, the select comes afterwards)
      x[r] = side ? from_up : up;
    }
    if (!side) {
      mphi = newton_norm_phi(0.0, x[N]);
      if (q == 0) {
#pragma unroll
        for (int p = 0; p < VP; ++p) {
          d2 v;
          v[0] = x[2 * p];
          v[1] = 2 * p + 1 < NB ? x[2 * p + 1 < NB ? 2 * p + 1 : 0] : 0.0;
          XS(m, p) = v;
        }
      }
    }
    {
      const int nb_ = n_dn > m ? n_dn : m;
      auto bwd_row = [&](int s) { return side ? (s < n_dn ? m + 1 + s : nx - 2) : (s < m ? m - 1 - s : 0); };
      // The records do not depend on the solution, so they are requested BD rows ahead into a ring of BD register buffers (compile-time
      // indices: the loop is unrolled BD times); vector memory operations complete in order, so consuming buffer d waits for its own
      // loads only.
      constexpr int BD = PREFETCH_ROWS<W>;
      d2 Rb[BD][RP];
#pragma unroll
      for (int d = 0; d < BD; ++d)
#pragma unroll
        for (int p = 0; p < RP; ++p) {       // (pairs of columns that do not exist are never loaded: they stay zero)
          Rb[d][p][0] = 0.0;
          Rb[d][p][1] = 0.0;
        }
#pragma unroll
      for (int d = 0; d < BD; ++d) {
        if (d < nb_) {
          const int i = bwd_row(d);
#pragma unroll
          for (int p = 0; p < RP; ++p)
            if (p < rp_valid) Rb[d][p] = __builtin_nontemporal_load(&REC(i, p));
        }
      }
      for (int s0 = 0; s0 < nb_; s0 += BD) {
#pragma unroll
       for (int d = 0; d < BD; ++d) {
        const int s = s0 + d;
        if (s >= nb_) break;
        const bool act = side ? s < n_dn : s < m;
        const int i = bwd_row(s);
        d2 R[RP];
#pragma unroll
        for (int p = 0; p < RP; ++p) R[p] = Rb[d][p];
        if (s + BD < nb_) {
          const int in = bwd_row(s + BD);
#pragma unroll
          for (int p = 0; p < RP; ++p)
            if (p < rp_valid) Rb[d][p] = __builtin_nontemporal_load(&REC(in, p));
        }
        if (act) {
          // this lane's share of t - T x: its columns (column NB is t itself)
          double y[NB];
#pragma unroll
          for (int r = 0; r < NB; ++r) y[r] = 0.0;
#pragma unroll
          for (int jj = 0; jj < CL; ++jj) {
            const int j = col_j(jj);
            const double xj = pick([&](int k) { return x[k]; }, jj, NB);
            const double w = j == NB ? 1.0 : (j < NB ? -xj : 0.0);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
              const double rv = j <= NB ? R[(jj * NB + r) >> 1][(jj * NB + r) & 1] : 0.0;      // (a pair may straddle into a column that does not exist)
              y[r] = __builtin_fma(rv, w, y[r]);
            }
          }
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            y[r] = col_sum<W>(y[r]);
            x[r] = y[r];
          }
          if (q == 0) {
#pragma unroll
            for (int p = 0; p < VP; ++p) {
              d2 v;
              v[0] = y[2 * p];
              v[1] = 2 * p + 1 < NB ? y[2 * p + 1 < NB ? 2 * p + 1 : 0] : 0.0;
              XS(i, p) = v;
            }
          }
          mphi = newton_norm_phi(mphi, y[N]);
        }
       }
      }
    }
    mphi = fmax(mphi, other_dir<W>(mphi));          // (the column lanes of a direction hold the same sums)
    const double lam = newton_damping(mphi, A.dphi_max);
#ifdef PNP_LANE_STAMPS
    const unsigned long long ts2 = __builtin_readcyclecounter();
#endif
    // =========================== update: the rows of a direction are split between its column lanes ================================================
    double upd = 0.0;
    {
      // upward direction: rows 0 .. m; downward direction: rows m+1 .. nx-1; column lane q takes every W-th row
      const int lo = side ? m + 1 : 0, cnt = side ? n_dn + 1 : m + 1;
      const int nu_ = ((n_dn + 1 > m + 1 ? n_dn + 1 : m + 1) + W - 1) / W;
      auto upd_row = [&](int s) { const int z = W * s + q; return lo + (z < cnt ? z : cnt - 1); };
      // (requested UD rows ahead, like the records of the backward pass)
      constexpr int UD = PREFETCH_ROWS<W>;
      d2 xb[UD][VP], cb2[UD][VP];
#pragma unroll
      for (int d = 0; d < UD; ++d) {
        const int i = upd_row(d);          // (clamped to the lane's last row beyond its share: a valid address)
#pragma unroll
        for (int p = 0; p < VP; ++p) {
          xb[d][p] = XS(i, p);
          cb2[d][p] = TS(i, p);
        }
      }
      for (int s0 = 0; s0 < nu_; s0 += UD) {
#pragma unroll
       for (int d = 0; d < UD; ++d) {
        const int s = s0 + d;
        if (s >= nu_) break;
        const bool act = W * s + q < cnt;
        const int i = upd_row(s);
        d2 x2[VP], c2[VP];
#pragma unroll
        for (int p = 0; p < VP; ++p) {
          x2[p] = xb[d][p];
          c2[p] = cb2[d][p];
        }
        if (s + UD < nu_) {
          const int in = upd_row(s + UD);
#pragma unroll
          for (int p = 0; p < VP; ++p) {
            xb[d][p] = XS(in, p);
            cb2[d][p] = TS(in, p);
          }
        }
        if (act) {
          double du[NB], cc_[N], cn[N];
#pragma unroll
          for (int r = 0; r < NB; ++r) du[r] = x2[r >> 1][r & 1];
          [[maybe_unused]] double f_old = 0.0, f_new = 0.0;
#pragma unroll
          for (int k = 0; k < N; ++k) {
            cc_[k] = c2[k >> 1][k & 1];
            upd = newton_norm_species(upd, du[k], cc_[k], s_cb[k][o]);
            if constexpr (CLIPS_WITH_THE_NORM<W>) {
              cn[k] = newton_floor_step(lam, du[k], cc_[k]);
              if constexpr (MPB) {
                f_old = __builtin_fma(G.vol[k], cc_[k], f_old);
                f_new = __builtin_fma(G.vol[k], cn[k], f_new);
              }
            }
          }
          if constexpr (!CLIPS_WITH_THE_NORM<W>) {
            newton_clip_row<N, MPB>(lam, du, cc_, G.vol, cn);
          } else if constexpr (MPB) {
            double theta;
            if (newton_free_volume(f_old, f_new, theta)) {
#pragma unroll
              for (int k = 0; k < N; ++k) cn[k] = newton_backtrack(theta, cn[k], cc_[k]);
            }
          }
          if (have) {
            double out[2 * VP];
#pragma unroll
            for (int k = 0; k < N; ++k) out[k] = cn[k];
            out[N] = __builtin_fma(lam, du[N], c2[N >> 1][N & 1]);
            if (NB < 2 * VP) out[2 * VP - 1] = 0.0;
#pragma unroll
            for (int p = 0; p < VP; ++p) {
              d2 v;
              v[0] = out[2 * p];
              v[1] = out[2 * p + 1];
              TS(i, p) = v;
            }
          }
        }
       }
      }
    }
    upd = col_max<W>(upd);
    upd = fmax(upd, other_dir<W>(upd));
    upd = fmax(upd, mphi * A.vt_inv);
    alarm = fmax(alarm, other_dir<W>(alarm));          // (the column lanes of a direction saw the same pivots)
#ifdef PNP_LANE_STAMPS
    {   // diagnosis build (tools/probe/lane4_stamps.sh): cycles of the three passes of this iteration, summed per wave
      const unsigned long long ts3 = __builtin_readcyclecounter();
      stamp_f += (double)(ts1 - ts0);
      stamp_b += (double)(ts2 - ts1);
      stamp_u += (double)(ts3 - ts2);
      stamp_n += 1.0;
    }
#endif
    // =========================== bookkeeping (identical in the 2 W lanes of an operating point) ======================================================
    if (have) {
      const bool accept = newton_accept(lam, upd, upd_prev, A.tol, A.estimate);
      if (accept || it >= A.maxit) {
        total_it += accept ? it : A.maxit + 1;
        if (!accept) st = PNP_STATUS_MAXIT;
        step += 1;
        fresh = true;
        if (step >= A.nsteps) {
          have = false;
          if ((lane & (2 * W - 1)) == 0) {
            G.status[b] = alarm > 0.0 ? (int)PNP_STATUS_MAXIT : st;
            G.iters[b] = total_it;
          }
        }
      }
    }
  }
#ifdef PNP_LANE_STAMPS
  if (lane == 0 && slot + 3 < G.B) {      // per wave: mean cycles per iteration of the three passes, in place of four points' iteration counts
    G.iters[slot + 0] = (int32_t)(stamp_f / stamp_n);
    G.iters[slot + 1] = (int32_t)(stamp_b / stamp_n);
    G.iters[slot + 2] = (int32_t)(stamp_u / stamp_n);
    G.iters[slot + 3] = (int32_t)stamp_n;
    if (slot + 7 < G.B) {      // ... and the sections of a forward row, mean cycles per row
      G.iters[slot + 4] = (int32_t)(row_a / row_n);
      G.iters[slot + 5] = (int32_t)(row_d / row_n);
      G.iters[slot + 6] = (int32_t)(row_g / row_n);
      G.iters[slot + 7] = (int32_t)(row_s / row_n);
    }
  }
#endif
}

// ---- the launcher: chunks of the batch (launch_lane_chunks), then block size, mode and BDF flag as template arguments of the family's
// ---- kernel.  K::template kernel<NB, MODE, BDF>() is that kernel's address --------------------------------------------------------------
template <int W, typename K>
inline hipError_t launch_lane_cols(const NewtonArgs& a0, hipStream_t stream) {
  return with_block<6, 9>(a0.N + 1, [&](auto NB) {
    return launch_lane_chunks<ColLanes<W>::PG>(a0, stream, [&](const NewtonArgs& a, int64_t ng) {
      with_mode(newton_mode_lane(a.mpb, a.rt, a.convect), [&](auto M) {
        with_flag(a.bdf2 != 0, [&](auto BDF) {
          hipLaunchKernelGGL((K::template kernel<decltype(NB)::value, decltype(M)::value, decltype(BDF)::value>()), dim3((unsigned)ng), dim3(64), 0,
                             stream, a);
        });
      });
    });
  });
}

}  // namespace lane
}  // namespace pnp
