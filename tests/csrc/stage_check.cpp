// Host unit test of catint_amd/csrc/pnp_stage.h (tests/test_stage_layout.py compiles this file against that header alone and runs it):
// the layout of the staged inputs, their placement, and the placement of the output rows.  Plain asserts; any failure aborts.
#undef NDEBUG
#include <cassert>
#include <cstdio>

#include "pnp_stage.h"

using namespace pnp::post;

// the sizes of the tables behind the lane lists, in doubles: any value serves, odd ones move most
constexpr size_t TEAM_TABLE = 1237, KIN_TABLE = 455;
constexpr size_t GRID_TAIL = (8 + 1) * 8;   // (MAX_SPECIES + 1) rows of SPF constants

struct Table;   // a pointee type of its own, as the kernels' arguments have one

// ---- a mix of sizes: even starts, no overlap, declaration order, the total ------------------------------------------------------------
static void mix_of_sizes() {
  const size_t sizes[] = {0, 1, 7, 10, 0, 3, ((size_t)1 << 33) + 5, 2, 1};
  constexpr int NS = sizeof sizes / sizeof sizes[0];
  const double* member[NS] = {};
  Inputs in;
  size_t sum = 0;
  for (int i = 0; i < NS; ++i) {
    const int id = in.add(sizes[i], &member[i]);
    assert(id == i);
    sum += even(sizes[i]);
  }
  assert(in.count == NS && in.count <= Inputs::CAPACITY);
  assert(in.total == sum);
  size_t end = 0;
  for (int i = 0; i < NS; ++i) {
    assert(in.slot[i].n == sizes[i]);
    assert(in.slot[i].offset % 2 == 0);
    assert(in.slot[i].offset >= end);   // behind everything declared before it
    end = in.slot[i].offset + sizes[i];
  }
  assert(end <= in.total);
  std::vector<double> stage(64);
  assert(in.host(stage, 2) == stage.data() + in.slot[2].offset);
}

// ---- placement: exactly the declared members, whatever their pointee type; an undeclared member keeps its null ------------------------
struct Guarded {
  uint64_t g0;
  const double* a;
  uint64_t g1;
  const int64_t* lanes;
  uint64_t g2;
  const int32_t* bad;
  uint64_t g3;
  const Table* tab;
  uint64_t g4;
  const double* absent;   // declared only under a condition that does not hold
  uint64_t g5;
  double* untouched;      // never declared
  uint64_t g6;
};

static void placement() {
  constexpr uint64_t S = 0xa5a5a5a5a5a5a5a5ull;
  static double here = 0.0;
  Guarded k = {S, nullptr, S, nullptr, S, nullptr, S, nullptr, S, nullptr, S, &here, S};
  Inputs in;
  in.add(5, &k.a);
  in.add_unpadded(3, &k.lanes);
  in.add(2, &k.bad);
  const bool given = false;
  if (given) in.add(9, &k.absent);
  in.add_unpadded(TEAM_TABLE, &k.tab);
  assert(in.count == 4 && in.total == 6 + 3 + 2 + TEAM_TABLE);
  std::vector<double> device(in.total + 4);   // stands for the device buffer: only addresses inside it are formed
  const double* base = device.data();
  in.place(base);
  assert(k.a == base);
  assert((const void*)k.lanes == (const void*)(base + 6));
  assert((const void*)k.bad == (const void*)(base + 9));
  assert((const void*)k.tab == (const void*)(base + 11));
  assert(k.absent == nullptr);
  assert(k.untouched == &here);
  assert(k.g0 == S && k.g1 == S && k.g2 == S && k.g3 == S && k.g4 == S && k.g5 == S && k.g6 == S);
  // a second buffer (the context's buffer grew): every member moves with it
  const double* other = device.data() + 4;
  in.place(other);
  assert(k.a == other && (const void*)k.tab == (const void*)(other + 11) && k.absent == nullptr);
}

// ---- catcpl_solve: the declarations of couple/catcpl.hip against the offset chain they replaced --------------------------------------
struct CoupleArgs {
  const int64_t* lanes;
  const int32_t* badin;
  const double *wgt, *vol, *sp;
  const Table* tab;
  const double *g, *K, *Kc, *Kphi;
};

static void couple_chain(size_t nx, size_t N, size_t nn) {
  // the chain, as it stood
  const size_t grid_doubles = even(nx - 1) + even(nx) + GRID_TAIL;
  const size_t o_g = grid_doubles, o_K = o_g + even(nn * N), o_Kc = o_K + even(nn * N), o_Kp = o_Kc + even(nn * N * N), o_l = o_Kp + even(nn * N),
               o_b = o_l + nn, o_t = o_b + even((nn + 1) / 2), n_in = o_t + TEAM_TABLE;
  CoupleArgs a = {};
  Inputs in;
  in.add(nx - 1, &a.wgt);
  in.add(nx, &a.vol);
  in.add(GRID_TAIL, &a.sp);
  in.add(nn * N, &a.g);
  in.add(nn * N, &a.K);
  in.add(nn * N * N, &a.Kc);
  in.add(nn * N, &a.Kphi);
  in.add_unpadded(nn, &a.lanes);
  in.add((nn + 1) / 2, &a.badin);
  in.add_unpadded(TEAM_TABLE, &a.tab);
  assert(in.count <= Inputs::CAPACITY);
  assert(in.total == n_in);
  std::vector<double> device(in.total);   // stands for the device buffer: only addresses inside it are formed
  const double* buf = device.data();
  in.place(buf);
  assert(a.wgt == buf && a.vol == buf + even(nx - 1) && a.sp == buf + even(nx - 1) + even(nx));
  assert(a.g == buf + o_g && a.K == buf + o_K && a.Kc == buf + o_Kc && a.Kphi == buf + o_Kp);
  assert((const void*)a.lanes == (const void*)(buf + o_l));
  assert((const void*)a.badin == (const void*)(buf + o_b));
  assert((const void*)a.tab == (const void*)(buf + o_t));
}

// ---- the microkinetic libraries: the declarations of pnp_kin.h (stage_inputs) against the Stage chain they replaced ------------------
struct KinArgs {
  const int64_t* lanes;
  const double *cs, *phis, *phiM, *sigma, *off, *gamma, *theta;
};

static void kin_chain(size_t sn, size_t N, size_t R, size_t T, bool from_view, bool sigma, bool off, bool gamma, bool theta) {
  const size_t o_pm = 0;
  const size_t o_cs = o_pm + even(sn);
  const size_t o_ps = o_cs + (from_view ? 0 : even(sn * N));
  const size_t o_sg = o_ps + (from_view ? 0 : even(sn));
  const size_t o_off = o_sg + (sigma ? even(sn) : 0);
  const size_t o_gm = o_off + (off ? sn * R * 2 : 0);
  const size_t o_th = o_gm + (gamma ? even(sn * N) : 0);
  const size_t o_l = o_th + (theta ? even(sn * T) : 0);
  const size_t o_t = o_l + sn;
  const size_t n_in = o_t + KIN_TABLE;
  KinArgs a = {};
  const Table* tab = nullptr;
  Inputs in;
  in.add(sn, &a.phiM);
  if (!from_view) in.add(sn * N, &a.cs), in.add(sn, &a.phis);
  if (sigma) in.add(sn, &a.sigma);
  if (off) in.add(sn * R * 2, &a.off);
  if (gamma && N) in.add(sn * N, &a.gamma);
  if (theta) in.add(sn * T, &a.theta);
  in.add_unpadded(sn, &a.lanes);
  in.add_unpadded(KIN_TABLE, &tab);
  assert(in.count <= Inputs::CAPACITY - 5);   // cateis_solve declares five more behind them
  assert(in.total == n_in);
  std::vector<double> device(in.total);   // stands for the device buffer: only addresses inside it are formed
  const double* buf = device.data();
  in.place(buf);
  assert(a.phiM == buf + o_pm);
  assert(from_view ? (a.cs == nullptr && a.phis == nullptr) : (a.cs == buf + o_cs && a.phis == buf + o_ps));
  assert(sigma ? a.sigma == buf + o_sg : a.sigma == nullptr);
  assert(off ? a.off == buf + o_off : a.off == nullptr);
  assert((gamma && N) ? a.gamma == buf + o_gm : a.gamma == nullptr);
  assert(theta ? a.theta == buf + o_th : a.theta == nullptr);
  assert((const void*)a.lanes == (const void*)(buf + o_l));
  assert((const void*)tab == (const void*)(buf + o_t));
}

// ---- output rows: rows_doubles and place_rows agree, unwanted rows keep their null ------------------------------------------------------
static void rows() {
  double h[4];
  double *d0 = nullptr, *d1 = nullptr, *d2 = nullptr, *d3 = nullptr, *d4 = nullptr;
  const Row r[] = {{h, &d0, 3}, {nullptr, &d1, 8}, {h + 1, &d2, 0}, {h + 2, &d3, 4}, {h + 3, &d4, 1}};
  assert(rows_doubles(r) == 4 + 4 + 2);
  std::vector<double> device(rows_doubles(r));
  double* buf = device.data();
  double* end = place_rows(r, buf);
  assert(end == buf + rows_doubles(r));
  assert(d0 == buf && d1 == nullptr && d2 == nullptr && d3 == buf + 4 && d4 == buf + 8);
  const Row none[] = {{nullptr, &d1, 5}, {h, &d2, 0}};
  assert(rows_doubles(none) == 0 && place_rows(none, buf) == buf && d1 == nullptr && d2 == nullptr);
}

int main() {
  mix_of_sizes();
  placement();
  couple_chain(5, 2, 3);
  couple_chain(66, 8, 65);
  for (size_t sn : {(size_t)1, (size_t)65})
    for (int mask = 0; mask < 32; ++mask)
      for (size_t N : {(size_t)0, (size_t)3})
        kin_chain(sn, N, 5, 4, mask & 1, mask & 2, mask & 4, mask & 8, mask & 16);
  rows();
  puts("stage_check ok");
  return 0;
}
