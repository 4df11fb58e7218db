// Stand-alone driver of ipx_nd_order and ipx_nd_symbolic (csrc/nested_order.hip) for a sanitizer
// build of the host code: the 5-point graph of an nx x ny grid (with the diagonal, sorted
// columns) at several leaf sizes, a graph of isolated rows and small pieces, the empty graph and
// refused arguments, every result checked.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "ipx.h"

struct Graph {
  std::vector<int32_t> rowptr{0}, colidx;
  int32_t n() const { return (int32_t)rowptr.size() - 1; }
};

// order + symbolic; 0 when every structural property holds
static int analyse(const Graph &g, int32_t leaf, int *count_out) {
  const int32_t n = g.n();
  std::vector<int32_t> perm(n > 0 ? n : 1, -7), sn_ptr(n + 1, -7);
  const int ns = ipx_nd_order(n, g.rowptr.data(), g.colidx.data(), leaf, perm.data(), sn_ptr.data());
  if (ns < 0 || (n > 0 && ns < 1)) return 1;
  *count_out = ns;
  std::vector<int32_t> pos(n > 0 ? n : 1, -1), owner(n > 0 ? n : 1, -1);
  if (sn_ptr[0] != 0 || sn_ptr[ns] != n) return 2;
  for (int32_t p = 0; p < n; ++p) {
    if (perm[p] < 0 || perm[p] >= n || pos[perm[p]] >= 0) return 3;      // a permutation
    pos[perm[p]] = p;
  }
  for (int j = 0; j < ns; ++j) {
    if (sn_ptr[j + 1] <= sn_ptr[j]) return 4;
    for (int32_t p = sn_ptr[j]; p < sn_ptr[j + 1]; ++p) {
      owner[p] = j;
      if (p > sn_ptr[j] && perm[p] <= perm[p - 1]) return 5;              // rows ascend
    }
  }
  std::vector<int32_t> parent(ns > 0 ? ns : 1), level(ns > 0 ? ns : 1);
  std::vector<int64_t> bnd_ptr(ns + 1);
  const int64_t total =
      ipx_nd_symbolic(n, g.rowptr.data(), g.colidx.data(), ns, perm.data(), sn_ptr.data(),
                      parent.data(), level.data(), bnd_ptr.data(), nullptr, nullptr, 0);
  if (total < 0 || bnd_ptr[ns] != total) return 6;
  std::vector<int32_t> bnd(total > 0 ? total : 1), cmap(total > 0 ? total : 1, -7);
  if (ipx_nd_symbolic(n, g.rowptr.data(), g.colidx.data(), ns, perm.data(), sn_ptr.data(),
                      parent.data(), level.data(), bnd_ptr.data(), bnd.data(), cmap.data(),
                      total) != total)
    return 7;
  for (int j = 0; j < ns; ++j) {
    const int64_t b0 = bnd_ptr[j], b1 = bnd_ptr[j + 1];
    if ((b1 == b0) != (parent[j] < 0)) return 8;
    // every neighbour of an own row is own, earlier, or on the boundary
    for (int32_t p = sn_ptr[j]; p < sn_ptr[j + 1]; ++p)
      for (int32_t e = g.rowptr[perm[p]]; e < g.rowptr[perm[p] + 1]; ++e) {
        const int32_t q = pos[g.colidx[e]];
        if (q < sn_ptr[j + 1]) continue;
        bool found = false;
        for (int64_t k = b0; k < b1; ++k) found = found || bnd[k] == q;
        if (!found) return 9;
      }
    if (parent[j] < 0) continue;
    const int pj = parent[j];
    if (pj <= j || level[pj] <= level[j] || owner[bnd[b0]] != pj) return 10;
    const int32_t s = sn_ptr[pj + 1] - sn_ptr[pj];
    for (int64_t k = b0; k < b1; ++k) {
      if (k > b0 && bnd[k] <= bnd[k - 1]) return 11;
      const int32_t at = cmap[k];
      const int32_t behind = at < s ? sn_ptr[pj] + at
                                    : (at - s < bnd_ptr[pj + 1] - bnd_ptr[pj]
                                           ? bnd[bnd_ptr[pj] + at - s] : -1);
      if (at < 0 || behind != bnd[k]) return 12;                          // the child map
    }
  }
  return 0;
}

int main() {
  const int nx = 37, ny = 23;
  Graph grid;
  for (int i = 0; i < ny; ++i)
    for (int j = 0; j < nx; ++j) {
      if (i > 0) grid.colidx.push_back((i - 1) * nx + j);
      if (j > 0) grid.colidx.push_back(i * nx + j - 1);
      grid.colidx.push_back(i * nx + j);
      if (j < nx - 1) grid.colidx.push_back(i * nx + j + 1);
      if (i < ny - 1) grid.colidx.push_back((i + 1) * nx + j);
      grid.rowptr.push_back((int32_t)grid.colidx.size());
    }
  const int n = nx * ny;
  const int leaves[] = {1, 4, 32, 64, n, n + 7};
  for (int leaf : leaves) {
    int count = 0;
    const int bad = analyse(grid, leaf, &count);
    if (bad || (leaf >= n && count != 1) || (leaf < 64 && count < n / (4 * leaf))) {
      printf("grid, leaf %d: count %d, check %d\n", leaf, count, bad);
      return 1;
    }
  }
  // pieces: an empty row, a row with its diagonal only, a pair, a path of 5 rows
  Graph pieces;
  const int32_t rp[] = {0, 0, 1, 3, 5, 7, 10, 13, 16, 18};
  const int32_t ci[] = {1, 2, 3, 2, 3, 4, 5, 4, 5, 6, 5, 6, 7, 6, 7, 8, 7, 8};
  pieces.rowptr.assign(rp, rp + 10);
  pieces.colidx.assign(ci, ci + 18);
  for (int leaf : {1, 2, 3, 16}) {
    int count = 0;
    const int bad = analyse(pieces, leaf, &count);
    if (bad || (leaf == 16 && count != 1)) {
      printf("pieces, leaf %d: count %d, check %d\n", leaf, count, bad);
      return 1;
    }
  }
  Graph empty;
  int count = -1;
  if (analyse(empty, 8, &count) || count != 0) {
    printf("empty graph\n");
    return 1;
  }
  // refused: leaf < 1, a column out of range, a row pointer that descends
  std::vector<int32_t> perm(9), sn_ptr(10);
  std::vector<int32_t> bad_ci(ci, ci + 18);
  bad_ci[17] = 9;
  std::vector<int32_t> bad_rp(rp, rp + 10);
  bad_rp[4] = 2;
  if (ipx_nd_order(9, rp, ci, 0, perm.data(), sn_ptr.data()) >= 0 ||
      ipx_nd_order(9, rp, bad_ci.data(), 4, perm.data(), sn_ptr.data()) >= 0 ||
      ipx_nd_order(9, bad_rp.data(), ci, 4, perm.data(), sn_ptr.data()) >= 0) {
    printf("bad arguments accepted\n");
    return 1;
  }
  printf("nested ok\n");
  return 0;
}
