// sweep.cpp -- the index arithmetic of the addition / transposition kernel (csrc/device/geadd_map.hpp) against
// brute-force models, on the CPU.  The program walks every work unit and every access of every thread exactly as
// kernels_geadd.hip does -- the same functions, the same order: load phase, LDS image, store phase -- over a memory made
// of element IDs, and checks
//   - every element of the uplo part inside the local extents is written exactly once, nothing else is written;
//   - the value that lands in a destination element is the right source element for N and T / C, on one process and
//     inside the class layout of the panel buffer that bcast_transposed_panel_whole fills on a grid;
//   - no access leaves the nb x nb storage of a tile;
//   - the vector / element decision against the alignment of every tile column;
//   - for the in-place completion: no element written by one work unit is read or written by another;
//   - the LDS image is a bijection, and its bank conflicts by the rule of the hardware guide.
// Output: counts, the conflict table, and "failures N".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "distribution.hpp"
#include "geadd_map.hpp"

using namespace dlaf_mi355x;

static long failures = 0, elements = 0, units_run = 0, panel_tiles = 0, inplace_units = 0, decisions = 0;
static void fail(const char* what, long a, long b, long c, long d) {
  if (failures < 20)
    std::printf("FAIL %s %ld %ld %ld %ld\n", what, a, b, c, d);
  ++failures;
}

struct Launch {
  GeaddGeom g;
  int mask, trans, ve, B;
  long a_tsi, a_ts, a_ts2;
  int a_period;
};

// One launch of the kernel over ID memory.  src: the source storage (element IDs), dst: destination storage, receives
// the ID of the source element; reads[i] / writes[i]: the work unit (1-based) that touched source / destination element
// i (in place: one array space); -2: touched by more than one unit.
struct Trace {
  std::vector<long>* dst;
  const std::vector<long>* src;
  std::vector<int>*reader, *writer;  // may be null
};
static void note(std::vector<int>* v, long i, int unit) {
  if (!v)
    return;
  int& s = (*v)[(size_t) i];
  s = (s == 0 || s == unit) ? unit : -2;
}
static void run_launch(const Launch& L, const Trace& t, long c_tsr, long c_tsc, int unit_base) {
  const int B = L.B, ve = L.ve, nb = L.g.nb;
  const int nsb = geadd_sub_blocks(nb, B), nv = B * B / ve;
  std::vector<long> lds((size_t) B * B);
  for (int jl = 0; jl < L.g.ltc; ++jl)
    for (int il = L.g.il0; il < L.g.il0 + L.g.nil; ++il)
      for (int sb = 0; sb < nsb * nsb; ++sb) {
        const int bi = sb % nsb, bj = sb / nsb;
        const GeaddUnit u = geadd_unit(L.g, L.mask, B, il, jl, bi, bj);
        if (u.cls == kGeaddDead)
          continue;
        ++units_run;
        const int unit = unit_base + 1 + sb + nsb * nsb * (il + L.g.ltr * jl);
        const long ct = (long) il * c_tsr + (long) jl * c_tsc;
        const long at = geadd_src_tile_offset(L.g, il, jl, L.a_tsi, L.a_period, L.a_ts, L.a_ts2);
        auto read_src = [&](int r, int c) -> long {  // element (r, c) of the source tile
          if (r < 0 || r >= nb || c < 0 || c >= nb) {
            fail("source access outside the tile", r, c, nb, unit);
            return -1;
          }
          const long i = at + geadd_src_elem(false, r, c, nb);
          if (i < 0 || i >= (long) t.src->size()) {
            fail("source access outside the storage", i, (long) t.src->size(), il, jl);
            return -1;
          }
          note(t.reader, i, unit);
          return (*t.src)[(size_t) i];
        };
        auto put = [&](int r, int c, const long* x) {
          const int rend = u.r0 + u.nr;
          const long gr = u.gr0 + (r - u.r0), gc = u.gc0 + (c - u.c0);
          const bool whole = geadd_vector_whole(L.mask, u.cls, ve, r, rend, gr, gc);
          for (int e = 0; e < ve; ++e)
            if (whole || geadd_element_written(L.mask, u.cls, r, e, rend, gr, gc)) {
              if (r + e >= nb || c >= nb) {
                fail("destination access outside the tile", r + e, c, nb, unit);
                continue;
              }
              const long i = ct + (r + e) + (long) c * nb;
              if ((*t.dst)[(size_t) i] != -1 && t.writer == nullptr)
                fail("element written twice", il, jl, r + e, c);
              (*t.dst)[(size_t) i] = x[e];
              note(t.writer, i, unit);
            }
        };
        long x[4];
        if (!L.trans) {
          for (int v = 0; v < nv; ++v) {
            const int lr = geadd_vec_row(ve, B, v), lc = geadd_vec_col(ve, B, v);
            if (lr < u.nr && lc < u.nc) {
              for (int e = 0; e < ve; ++e)
                x[e] = read_src(u.r0 + lr + e, u.c0 + lc);
              put(u.r0 + lr, u.c0 + lc, x);
            }
          }
        }
        else {
          std::fill(lds.begin(), lds.end(), -7);
          for (int v = 0; v < nv; ++v) {
            const int sr = geadd_vec_row(ve, B, v), sc = geadd_vec_col(ve, B, v);
            if (sr < u.nc && sc < u.nr)
              for (int e = 0; e < ve; ++e)
                lds[(size_t) geadd_lds_index(ve, B, sr, sc) + e] = read_src(u.c0 + sr + e, u.r0 + sc);
          }
          for (int v = 0; v < nv; ++v) {
            const int lr = geadd_vec_row(ve, B, v), lc = geadd_vec_col(ve, B, v);
            if (lr < u.nr && lc < u.nc) {
              for (int e = 0; e < ve; ++e)
                x[e] = lds[(size_t) geadd_lds_index(ve, B, lc, lr + e)];
              put(u.r0 + lr, u.c0 + lc, x);
            }
          }
        }
      }
}

static GeaddGeom geom_of(const Axis& rows, const Axis& cols) {
  GeaddGeom g;
  g.ltr = (int) rows.local_tiles();
  g.ltc = (int) cols.local_tiles();
  g.nb = rows.nb;
  g.rows = rows.local_size();
  g.cols = cols.local_size();
  g.pr = rows.P;
  g.ri = rows.shift();
  g.pc = cols.P;
  g.ci = cols.shift();
  g.il0 = 0;
  g.nil = g.ltr;
  return g;
}

// the destination after the launches against the model: element (i, j) of the m x n matrix C takes the ID that
// want_id(i, j) names, when it is in the part and local; everything else stays -1
template <class WantId>
static void check_dest(const std::vector<long>& dst, const Axis& rows, const Axis& cols, int mask, WantId want_id) {
  const int nb = rows.nb;
  const long ltr = rows.local_tiles(), ltc = cols.local_tiles();
  for (long jl = 0; jl < ltc; ++jl)
    for (long il = 0; il < ltr; ++il)
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const long gi = rows.global_of(il) * nb + r, gj = cols.global_of(jl) * nb + c;
          const bool inside = gi < rows.n && gj < cols.n && geadd_element_in(mask, gi, gj);
          const long got = dst[(size_t) ((il + jl * ltr) * nb * nb + r + (long) c * nb)];
          ++elements;
          if (!inside) {
            if (got != -1)
              fail("written outside the part", gi, gj, got, mask);
          }
          else if (got != want_id(gi, gj))
            fail("wrong source element", gi, gj, got, want_id(gi, gj));
        }
}

// one process (P = Q = 1) or the local op N launch of a grid: source and destination share the distribution
static void sweep_local(long m, long n, int nb, int P, int Q, int p, int q, int isrc, int jsrc, int mask, bool trans,
                        int ve, int B) {
  Axis rows{m, nb, P, p, isrc}, cols{n, nb, Q, q, jsrc};
  const long te = (long) nb * nb, ltr = rows.local_tiles(), ltc = cols.local_tiles();
  if (ltr == 0 || ltc == 0)
    return;
  Launch L{geom_of(rows, cols), mask, trans ? 1 : 0, ve, B, 0, 0, 0, 1};
  // the source as stored: m x n with C's distribution (op N), or n x m on ONE process (op T: tile (jl, il))
  const long sltr = trans ? ltc : ltr, sltc = trans ? ltr : ltc;
  L.a_tsi = trans ? te * sltr : te;
  L.a_ts = trans ? te : te * sltr;
  std::vector<long> src((size_t) (sltr * sltc * te)), dst((size_t) (ltr * ltc * te), -1);
  // ID of element (r, c) of source tile (I, J): its global coordinates in the source matrix, or -3 in the padding
  const Axis& srows = trans ? cols : rows;
  const Axis& scols = trans ? rows : cols;
  for (long J = 0; J < sltc; ++J)
    for (long I = 0; I < sltr; ++I)
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const long gi = srows.global_of(I) * nb + r, gj = scols.global_of(J) * nb + c;
          src[(size_t) ((I + J * sltr) * te + r + (long) c * nb)] = (gi < srows.n && gj < scols.n) ? gi * 100000 + gj : -3;
        }
  Trace t{&dst, &src, nullptr, nullptr};
  run_launch(L, t, te, te * ltr, 0);
  check_dest(dst, rows, cols, mask, [&](long gi, long gj) { return trans ? gj * 100000 + gi : gi * 100000 + gj; });
}

static long gcd_of(long a, long b) {
  while (b) {
    const long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// op T on a P x Q grid, process (p, q): for every tile column k of A (n x m) whose tile row of C this process row owns,
// one launch over that row from a panel buffer laid out as bcast_transposed_panel_whole(have = A's rows, want = C's
// columns) leaves it: the model groups the local tile columns by root process in order of first appearance
static void sweep_panel(long m, long n, int nb, int P, int Q, int p, int q, int c_isrc, int c_jsrc, int a_isrc, int mask,
                        int ve, int B) {
  Axis crows{m, nb, P, p, c_isrc}, ccols{n, nb, Q, q, c_jsrc};
  Axis have{n, nb, P, p, a_isrc};  // A's rows: the n dimension over the process rows
  const Axis& want = ccols;
  const long te = (long) nb * nb, ltr = crows.local_tiles(), ltc = ccols.local_tiles();
  if (ltr == 0 || ltc == 0)
    return;
  const bool hop = have.P > 1;
  // what the library computes (sweep.hpp)
  int period = 1;
  long ts = te, ts2 = 0, base = 0, buf_tiles;
  if (hop) {
    const long g = gcd_of(have.P, want.P);
    period = (int) (have.P / g);
    ts2 = ((ltc + period - 1) / period) * te;
    buf_tiles = ltc + have.P;
  }
  else {
    base = (long) want.shift() * te;
    ts = te * want.P;
    buf_tiles = have.nt();
  }
  // the model of the buffer: where the panel's tile of global row gj = want.global_of(jl) lies
  std::vector<long> model_off((size_t) ltc);
  if (hop) {
    std::vector<int> roots;
    std::vector<long> count;
    long cap = 0;
    std::vector<int> cls((size_t) ltc);
    std::vector<long> pos((size_t) ltc);
    for (long jl = 0; jl < ltc; ++jl) {
      const int root = have.owner(want.global_of(jl));
      size_t c = 0;
      while (c < roots.size() && roots[c] != root)
        ++c;
      if (c == roots.size()) {
        roots.push_back(root);
        count.push_back(0);
      }
      cls[(size_t) jl] = (int) c;
      pos[(size_t) jl] = count[c]++;
      cap = std::max(cap, count[c]);
    }
    for (long jl = 0; jl < ltc; ++jl)
      model_off[(size_t) jl] = cls[(size_t) jl] * cap * te + pos[(size_t) jl] * te;
  }
  else {
    for (long jl = 0; jl < ltc; ++jl)
      model_off[(size_t) jl] = want.global_of(jl) * te;
  }
  std::vector<long> dst((size_t) (ltr * ltc * te), -1);
  for (long k = 0; k < crows.nt(); ++k) {
    if (!crows.mine(k))
      continue;
    // the buffer of step k: tile jl holds A(gj, k), element (r, c) = A(gj nb + r, k nb + c); A is n x m
    std::vector<long> buf((size_t) (buf_tiles * te), -5);
    for (long jl = 0; jl < ltc; ++jl) {
      ++panel_tiles;
      const long gj = want.global_of(jl);
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const long ai = gj * nb + r, aj = k * nb + c;
          buf[(size_t) (model_off[(size_t) jl] + r + (long) c * nb)] = (ai < n && aj < m) ? ai * 100000 + aj : -3;
        }
    }
    Launch L{geom_of(crows, ccols), mask, 1, ve, B, 0, ts, ts2, period};
    L.g.il0 = (int) crows.local_of(k);
    L.g.nil = 1;
    // (the base of the no-hop form is added to the pointer by the host: model it by shifting the buffer view)
    std::vector<long> view(buf.begin() + base, buf.end());
    Trace t{&dst, &view, nullptr, nullptr};
    run_launch(L, t, te, te * ltr, 0);
  }
  check_dest(dst, crows, ccols, mask, [&](long gi, long gj) { return gj * 100000 + gi; });
}

// hermitian_complete in place on one process: source = destination; across work units no written element may be read
// or written by another unit
static void sweep_in_place(long n, int nb, bool upper_stored, bool herm, int ve, int B) {
  Axis rows{n, nb, 1, 0, 0}, cols{n, nb, 1, 0, 0};
  const long te = (long) nb * nb, lt = rows.local_tiles();
  const int mask = herm ? (upper_stored ? kGeaddLowerEq : kGeaddUpperEq) : (upper_stored ? kGeaddLower : kGeaddUpper);
  Launch L{geom_of(rows, cols), mask, 1, ve, B, te * lt, te, 0, 1};
  std::vector<long> mem((size_t) (lt * lt * te));
  for (long J = 0; J < lt; ++J)
    for (long I = 0; I < lt; ++I)
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const long gi = I * nb + r, gj = J * nb + c;
          mem[(size_t) ((I + J * lt) * te + r + (long) c * nb)] = (gi < n && gj < n) ? gi * 100000 + gj : -3;
        }
  const std::vector<long> before = mem;
  std::vector<long> out = mem;
  std::vector<int> reader(mem.size(), 0), writer(mem.size(), 0);
  Trace t{&out, &before, &reader, &writer};  // every unit reads the ORIGINAL: valid only if the sets are disjoint
  const long u0 = units_run;
  run_launch(L, t, te, te * lt, 0);
  inplace_units += units_run - u0;
  for (size_t i = 0; i < mem.size(); ++i) {
    if (writer[i] == -2)
      fail("in place: element written by two units", (long) i, n, nb, mask);
    if (writer[i] != 0 && reader[i] != 0 && reader[i] != writer[i])
      fail("in place: element written by one unit and read by another", (long) i, n, nb, mask);
  }
  for (long J = 0; J < lt; ++J)
    for (long I = 0; I < lt; ++I)
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const long gi = I * nb + r, gj = J * nb + c;
          const size_t i = (size_t) ((I + J * lt) * te + r + (long) c * nb);
          ++elements;
          const bool inside = gi < n && gj < n && geadd_element_in(mask, gi, gj);
          if (inside ? out[i] != gj * 100000 + gi : out[i] != before[i])
            fail("in place: wrong element", gi, gj, out[i], mask);
        }
}

// lane groups of a wave per access kind (MI355X: the hardware guide's LDS table)
static int worst_conflict(const std::vector<long>& byte_addr, int access_bytes, int modulus,
                          const std::vector<std::vector<int>>& groups) {
  int worst = 1;
  for (const auto& grp : groups) {
    std::vector<std::vector<long>> bank((size_t) modulus);
    for (int lane : grp) {
      if (byte_addr[(size_t) lane] < 0)
        continue;
      for (int d = 0; d < access_bytes / 4; ++d) {
        auto& b = bank[(size_t) ((byte_addr[(size_t) lane] / 4 + d) % modulus)];
        const long a = byte_addr[(size_t) lane] + 4 * d;
        if (std::find(b.begin(), b.end(), a) == b.end())
          b.push_back(a);
      }
    }
    for (const auto& b : bank)
      worst = std::max(worst, (int) b.size());
  }
  return worst;
}
static std::vector<std::vector<int>> contiguous_groups(int size) {
  std::vector<std::vector<int>> g;
  for (int l0 = 0; l0 < 64; l0 += size) {
    g.emplace_back();
    for (int l = l0; l < l0 + size; ++l)
      g.back().push_back(l);
  }
  return g;
}
static std::vector<std::vector<int>> b128_read_groups() {
  auto range = [](std::vector<int>& v, int a, int b) {
    for (int l = a; l <= b; ++l)
      v.push_back(l);
  };
  std::vector<std::vector<int>> g(4);
  range(g[0], 0, 3), range(g[0], 12, 15), range(g[0], 20, 27);
  range(g[1], 4, 11), range(g[1], 16, 19), range(g[1], 28, 31);
  range(g[2], 32, 35), range(g[2], 44, 47), range(g[2], 52, 59);
  range(g[3], 36, 43), range(g[3], 48, 51), range(g[3], 60, 63);
  return g;
}
static void lds_report(const char* name, int eb, int ve) {
  const int B = geadd_block(eb), nv = B * B / ve;
  // bijection
  std::vector<int> seen((size_t) B * B, 0);
  for (int sc = 0; sc < B; ++sc)
    for (int sr = 0; sr < B; ++sr) {
      const int i = geadd_lds_index(ve, B, sr, sc);
      if (i < 0 || i >= B * B || seen[(size_t) i]++)
        fail("LDS image is no bijection", eb, ve, sr, sc);
      if (sr % ve == 0 && i % ve != 0)
        fail("LDS slot misaligned", eb, ve, sr, sc);
    }
  int w_store = 1, w_load = 1, w_load2 = 1;
  for (int wave0 = 0; wave0 < nv; wave0 += 64) {
    std::vector<long> a(64);
    // store side: one access of ve elements per lane (8-lane groups for 16 bytes, 16 for 8, 32 for 4; bank mod 32)
    for (int l = 0; l < 64; ++l) {
      const int v = wave0 + l;
      a[(size_t) l] = (long) geadd_lds_index(ve, B, geadd_vec_row(ve, B, v), geadd_vec_col(ve, B, v)) * eb;
    }
    const int sbytes = ve * eb;
    w_store = std::max(w_store, worst_conflict(a, sbytes, 32, contiguous_groups(sbytes == 16 ? 8 : sbytes == 8 ? 16 : 32)));
    // load side: one element per lane and e; as single reads (b32 mod 32 / b64, b128 mod 64) and as the paired
    // ds_read2st64 the compiler makes of two consecutive columns (mod 32; 16-lane groups for 8-byte elements)
    for (int e = 0; e < ve; ++e) {
      for (int l = 0; l < 64; ++l) {
        const int v = wave0 + l;
        a[(size_t) l] = (long) geadd_lds_index(ve, B, geadd_vec_col(ve, B, v), geadd_vec_row(ve, B, v) + e) * eb;
      }
      w_load = std::max(w_load, worst_conflict(a, eb, eb == 4 ? 32 : 64, eb == 16 ? b128_read_groups() : contiguous_groups(32)));
      w_load2 = std::max(w_load2, worst_conflict(a, eb, 32, contiguous_groups(eb == 4 ? 32 : 16)));
    }
  }
  std::printf("lds %s ve %d B %d: store %d-way, load %d-way (paired reads: %d-way)\n", name, ve, B, w_store, w_load, w_load2);
  if (ve * eb == 16 && (w_store > 2 || w_load > 2 || (eb < 16 && w_load2 > 2)))
    fail("LDS image more than 2-way conflicted", eb, ve, w_store, w_load);
}

int main() {
  // ---- the vector / element decision against the alignment of every tile column and tile base
  for (int eb : {4, 8, 16})
    for (int nb = 1; nb <= 170; ++nb)
      for (unsigned long long a_off : {0ull, 4ull, 8ull, 16ull})
        for (unsigned long long c_off : {0ull, 8ull, 16ull}) {
          if (a_off % eb || c_off % eb)
            continue;
          const unsigned long long a = 4096 + a_off, c = 8192 + c_off;
          bool ok = true;
          for (int t = 0; t < 3; ++t)
            for (int col = 0; col < nb; ++col) {
              const unsigned long long off = ((unsigned long long) t * nb * nb + (unsigned long long) col * nb) * eb;
              ok = ok && (a + off) % 16 == 0 && (c + off) % 16 == 0;
            }
          const int want = (ok && eb < 16) ? 16 / eb : 1;
          ++decisions;
          if (geadd_vector_elems(eb, nb, a, c) != want)
            fail("vector decision", eb, nb, (long) a_off, (long) c_off);
        }
  // ---- one process: every tile size, both forms, every mask, vector and element path, two rectangular shapes
  for (int eb : {4, 8, 16}) {
    const int B = geadd_block(eb), vmax = eb < 16 ? 16 / eb : 1;
    for (int nb = 1; nb <= 170; ++nb)
      for (int ve : {1, vmax}) {
        if (ve > 1 && nb % ve != 0)
          continue;  // (the decision above: such a tile takes the element path)
        if (ve == 1 && vmax > 1 && nb % vmax == 0 && nb % 3 != 0)
          continue;  // the element path of an alignable size: every third size is enough
        for (int mask = 0; mask <= 4; ++mask)
          for (int trans = 0; trans <= 1; ++trans) {
            const int r1 = 1 + nb / 2, r2 = 1 + (2 * nb) / 3;  // ragged last tiles
            sweep_local(nb + r1, nb + r2, nb, 1, 1, 0, 0, 0, 0, mask, trans != 0, ve, B);
            sweep_local(nb + r2, nb, nb, 1, 1, 0, 0, 0, 0, mask, trans != 0, ve, B);
          }
      }
  }
  sweep_local(1, 300, 160, 1, 1, 0, 0, 0, 0, kGeaddUpperEq, true, 2, 64);
  sweep_local(300, 1, 160, 1, 1, 0, 0, 0, 0, kGeaddLowerEq, true, 2, 64);
  // ---- grids up to 2 x 3, every process, every source process: the local op N launch and the panel-buffer op T
  for (int nb = 1; nb <= 170; ++nb) {
    const int eb = 8, B = geadd_block(eb), ve = nb % 2 == 0 ? 2 : 1;
    const int grids[4][2] = {{1, 2}, {2, 1}, {2, 2}, {2, 3}};
    {
      // (the grid shapes take turns over the tile sizes: each shape meets every residue of nb modulo the vector width
      // and the sub-block)
      const int P = grids[nb % 4][0], Q = grids[nb % 4][1];
      // more tile rows than process rows; 2 or 3 local tile columns, so that the classes of the panel differ in length
      const long m = (P + 1L) * nb + 1 + nb / 2, n = 2L * Q * nb + 1 + nb / 3;
      for (int isrc = 0; isrc < P; ++isrc)
        for (int jsrc = 0; jsrc < Q; ++jsrc)
          for (int p = 0; p < P; ++p)
            for (int q = 0; q < Q; ++q) {
              const int mask = (nb + isrc + 2 * jsrc) % 3;  // A, L, U in turn
              sweep_local(m, n, nb, P, Q, p, q, isrc, jsrc, mask, false, ve, B);
              // (A starts on another process row than C wherever there is one)
              sweep_panel(m, n, nb, P, Q, p, q, isrc, jsrc, (isrc + 1) % P, (mask + 1) % 3, ve, B);
            }
    }
  }
  // ---- hermitian_complete in place: read and write sets of the work units
  for (int eb : {4, 8, 16}) {
    const int B = geadd_block(eb), vmax = eb < 16 ? 16 / eb : 1;
    for (int nb = 1; nb <= 170; ++nb) {
      const int ve = nb % vmax == 0 ? vmax : 1;
      const long n = 2L * nb + 1 + nb / 3;
      for (int upper = 0; upper <= 1; ++upper)
        for (int herm = 0; herm <= 1; ++herm)
          sweep_in_place(n, nb, upper != 0, herm != 0, ve, B);
      if (nb % 17 == 0)
        sweep_in_place(nb, nb, false, true, 1, B);
    }
  }
  // ---- the LDS image
  lds_report("float", 4, 4);
  lds_report("double / complex float", 8, 2);
  lds_report("complex double", 16, 1);
  lds_report("float, element path", 4, 1);
  lds_report("double, element path", 8, 1);
  std::printf("elements %ld units %ld panel_tiles %ld inplace_units %ld decisions %ld failures %ld\n", elements, units_run,
              panel_tiles, inplace_units, decisions, failures);
  return failures == 0 ? 0 : 1;
}
