// Nested-dissection order and supernodal symbolic factorization of S = A A' for the sparse direct
// solver (ipsolver/nested.py; csrc/nested.hip).  Host code only: no device calls.  include/ipx.h
// has the rules; tests/nested_model.py is the same in numpy.
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../include/ipx.h"

namespace {

struct Dissector {
  int32_t n, leaf;
  const int32_t *rowptr, *colidx;
  std::vector<int32_t> part;      // the part a row is in now (a stamp)
  std::vector<int32_t> seen;      // the stamp of the breadth-first search that reached a row
  std::vector<int32_t> lev;       // its level in that search
  int32_t stamp = 0, search = 0;
  int32_t *perm, *sn_ptr;
  int32_t count = 0, filled = 0;

  void emit(std::vector<int32_t> &rows) {
    std::sort(rows.begin(), rows.end());
    for (int32_t r : rows) perm[filled++] = r;
    sn_ptr[++count] = filled;
  }

  // rows of part `id` reached from `start`, in the order reached; lev[] holds their levels
  void levels(int32_t id, int32_t start, std::vector<int32_t> &out) {
    out.clear();
    ++search;
    seen[start] = search;
    lev[start] = 0;
    out.push_back(start);
    for (size_t head = 0; head < out.size(); ++head) {
      const int32_t i = out[head];
      for (int32_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
        const int32_t j = colidx[p];
        if (part[j] == id && seen[j] != search) {
          seen[j] = search;
          lev[j] = lev[i] + 1;
          out.push_back(j);
        }
      }
    }
  }

  // rows: ascending
  void dissect(std::vector<int32_t> &rows) {
    if ((int32_t)rows.size() <= leaf) return emit(rows);
    int32_t id = ++stamp;
    for (int32_t r : rows) part[r] = id;
    std::vector<int32_t> reached;
    levels(id, rows[0], reached);
    if (reached.size() < rows.size()) {               // not connected: piece by piece
      for (size_t at = 0; at < rows.size(); ++at) {
        if (part[rows[at]] != id) continue;           // (in a piece already taken)
        std::vector<int32_t> piece;
        levels(id, rows[at], piece);
        std::sort(piece.begin(), piece.end());
        dissect(piece);                               // (restamps its rows: they leave `id`)
        if ((int32_t)piece.size() <= leaf)
          for (int32_t r : piece) part[r] = -1;
      }
      return;
    }
    for (int pass = 0; pass < 2; ++pass) {
      const int32_t last = lev[reached.back()];
      int32_t start = n;
      for (size_t k = reached.size(); k-- > 0 && lev[reached[k]] == last;)
        start = std::min(start, reached[k]);
      levels(id, start, reached);
    }
    const int32_t nlev = lev[reached.back()] + 1;
    if (nlev < 3) return emit(rows);
    std::vector<int64_t> cum((size_t)nlev, 0);
    for (int32_t r : reached) ++cum[lev[r]];
    const int64_t half = ((int64_t)rows.size() + 1) / 2;
    int32_t cut = 0;
    for (int64_t sum = 0; cut < nlev; ++cut)
      if ((sum += cum[cut]) >= half) break;
    cut = std::min(std::max(cut, 1), nlev - 2);
    std::vector<int32_t> before, after, sep;
    for (int32_t r : reached) (lev[r] < cut ? before : lev[r] > cut ? after : sep).push_back(r);
    std::sort(before.begin(), before.end());
    std::sort(after.begin(), after.end());
    dissect(before);
    dissect(after);
    emit(sep);
  }
};

int bad_pattern(int64_t n, const int32_t *rowptr, const int32_t *colidx) {
  if (n < 0 || n > INT32_MAX / 2 || !rowptr) return 1;
  if (rowptr[0] != 0) return 1;
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return 1;
  if (n > 0 && rowptr[n] > 0 && !colidx) return 1;
  for (int32_t p = 0; n > 0 && p < rowptr[n]; ++p)
    if (colidx[p] < 0 || colidx[p] >= n) return 1;
  return 0;
}

}  // namespace

extern "C" {

int ipx_nd_order(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t leaf,
                 int32_t *perm, int32_t *sn_ptr) {
  if (leaf < 1 || !perm || !sn_ptr || bad_pattern(n, rowptr, colidx)) return IPX_EINVAL;
  Dissector d;
  d.n = (int32_t)n;
  d.leaf = leaf;
  d.rowptr = rowptr;
  d.colidx = colidx;
  d.part.assign((size_t)n, 0);
  d.seen.assign((size_t)n, 0);
  d.lev.assign((size_t)n, 0);
  d.perm = perm;
  d.sn_ptr = sn_ptr;
  sn_ptr[0] = 0;
  if (n > 0) {
    std::vector<int32_t> all((size_t)n);
    for (int32_t i = 0; i < (int32_t)n; ++i) all[i] = i;
    d.dissect(all);
  }
  return d.count;
}

int64_t ipx_nd_symbolic(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t nsuper,
                        const int32_t *perm, const int32_t *sn_ptr, int32_t *parent,
                        int32_t *level, int64_t *bnd_ptr, int32_t *bnd, int32_t *cmap,
                        int64_t cap) {
  if (nsuper < 0 || nsuper > n || !perm || !sn_ptr || !parent || !level || !bnd_ptr ||
      bad_pattern(n, rowptr, colidx))
    return IPX_EINVAL;
  if (sn_ptr[0] != 0 || sn_ptr[nsuper] != n) return IPX_EINVAL;
  std::vector<int32_t> pos((size_t)n, -1), owner((size_t)n);
  for (int64_t p = 0; p < n; ++p) {
    if (perm[p] < 0 || perm[p] >= n || pos[perm[p]] >= 0) return IPX_EINVAL;
    pos[perm[p]] = (int32_t)p;
  }
  for (int32_t j = 0; j < nsuper; ++j) {
    if (sn_ptr[j + 1] <= sn_ptr[j]) return IPX_EINVAL;
    for (int32_t p = sn_ptr[j]; p < sn_ptr[j + 1]; ++p) owner[p] = j;
  }
  std::vector<std::vector<int32_t>> bnds((size_t)nsuper), children((size_t)nsuper);
  std::vector<int32_t> mark((size_t)n, -1);
  int64_t total = 0;
  for (int32_t j = 0; j < nsuper; ++j) {
    const int32_t end = sn_ptr[j + 1];
    std::vector<int32_t> &b = bnds[j];
    parent[j] = -1;
    level[j] = 0;
    for (int32_t p = sn_ptr[j]; p < end; ++p) {
      const int32_t i = perm[p];
      for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int32_t q = pos[colidx[e]];
        if (q >= end && mark[q] != j) {
          mark[q] = j;
          b.push_back(q);
        }
      }
    }
    for (int32_t c : children[j]) {
      level[j] = std::max(level[j], level[c] + 1);
      for (int32_t q : bnds[c])
        if (q >= end && mark[q] != j) {
          mark[q] = j;
          b.push_back(q);
        }
    }
    std::sort(b.begin(), b.end());
    if (!b.empty()) {
      parent[j] = owner[b[0]];
      children[parent[j]].push_back(j);
    }
    bnd_ptr[j] = total;
    total += (int64_t)b.size();
  }
  bnd_ptr[nsuper] = total;
  if (!bnd || !cmap || cap < total) return total;
  for (int32_t j = 0; j < nsuper; ++j) {
    const std::vector<int32_t> &b = bnds[j];
    std::copy(b.begin(), b.end(), bnd + bnd_ptr[j]);
    const int32_t p = parent[j];
    if (p < 0) continue;
    const std::vector<int32_t> &pb = bnds[p];
    const int32_t s = sn_ptr[p + 1] - sn_ptr[p];
    for (size_t k = 0; k < b.size(); ++k) {
      const int32_t q = b[k];
      cmap[bnd_ptr[j] + (int64_t)k] =
          q < sn_ptr[p + 1] ? q - sn_ptr[p]
                            : s + (int32_t)(std::lower_bound(pb.begin(), pb.end(), q) - pb.begin());
    }
  }
  return total;
}

}  // extern "C"
