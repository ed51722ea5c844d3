// The layout of what an entry point moves between the host and the context's device buffer: the staged inputs of a call (`Inputs`) and
// the output rows behind them (`Row`).  Plain C++, no HIP: tests/csrc/stage_check.cpp compiles it alone.
//
// An entry point declares every staged input once, in the order it lies in the staging vector: its size in doubles and the member of
// the kernel's arguments that will hold its device address.  The inputs lie one behind the other from offset 0, each padded to an even
// count of doubles (16 bytes) unless it is declared unpadded.  After the device buffer is reserved -- reserve() frees and reallocates,
// so no address formed before it is valid -- `place` sets every declared member; no other code forms the device address of an input.
#pragma once
#include <cstddef>
#include <cstdint>
#include <new>
#include <vector>

namespace pnp {
namespace post {

static size_t even(size_t n) { return (n + 1) & ~(size_t)1; }

struct Inputs {
  static constexpr int CAPACITY = 20;   // the longest list (cateis_solve) has 14; add() does not check: stage_check.cpp counts
  struct Slot {
    size_t offset, n;   // doubles
    void* member;       // the pointer object in the kernel's arguments, of any pointee type
  };
  Slot slot[CAPACITY];
  int count = 0;
  size_t total = 0;   // doubles of all inputs declared so far: where the next one starts, and what is copied to the device

  // n doubles whose device address goes to *member; returns the slot, see host().  n = 0 occupies nothing (the member is still set)
  template <class T>
  int add(size_t n, T** member) {
    const int id = add_unpadded(n, member);
    total = slot[id].offset + even(n);
    return id;
  }
  // the same without the padding: the next input starts right behind this one (lane lists and what has always followed them)
  template <class T>
  int add_unpadded(size_t n, T** member) {
    slot[count] = Slot{total, n, member};
    total += n;
    return count++;
  }

  // where input `id` is written on the host, once the staging vector holds `total` doubles
  double* host(std::vector<double>& stage, int id) const { return stage.data() + slot[id].offset; }

  // every declared member points to its input in the copy at device_base
  void place(const double* device_base) const {
    for (int i = 0; i < count; ++i) {
      const double* at = device_base + slot[i].offset;
      __builtin_memcpy(slot[i].member, &at, sizeof at);   // whatever the pointee type of the member
    }
  }
};

// An output row: n doubles go to `host` from the device address the library's kernel arguments keep at *dev.  A row is wanted when
// the caller gave a pointer and it is not empty; the wanted rows lie one behind the other, each padded to an even count.
struct Row {
  double* host;
  double** dev;
  size_t n;
  bool wanted() const { return host && n; }
};

template <size_t NR>
static size_t rows_doubles(const Row (&rows)[NR]) {
  size_t need = 0;
  for (const Row& r : rows)
    if (r.wanted()) need += even(r.n);
  return need;
}

// sets *dev of the wanted rows from `cur` on; the first double behind them
template <size_t NR>
static double* place_rows(const Row (&rows)[NR], double* cur) {
  for (const Row& r : rows)
    if (r.wanted()) {
      *r.dev = cur;
      cur += even(r.n);
    }
  return cur;
}

}  // namespace post
}  // namespace pnp
