// Stand-alone driver of ipx_aggregate_greedy (csrc/aggregate.hip) for a sanitizer build of the
// host code: the 5-point graph of an nx x ny grid (with the diagonal, sorted columns), a graph
// with isolated rows, the empty graph and refused arguments, every result checked.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "ipx.h"

static int check(const std::vector<int32_t> &agg, int count, int cap) {
  std::vector<int> size(count > 0 ? count : 0, 0);
  for (int32_t a : agg) {
    if (a < 0 || a >= count) return 1;
    ++size[a];
  }
  for (int s : size)
    if (s < 1 || s > cap) return 2;
  return 0;
}

int main() {
  const int nx = 37, ny = 23, n = nx * ny;
  std::vector<int32_t> rowptr(1, 0), colidx;
  for (int i = 0; i < ny; ++i)
    for (int j = 0; j < nx; ++j) {
      if (i > 0) colidx.push_back((i - 1) * nx + j);
      if (j > 0) colidx.push_back(i * nx + j - 1);
      colidx.push_back(i * nx + j);
      if (j < nx - 1) colidx.push_back(i * nx + j + 1);
      if (i < ny - 1) colidx.push_back((i + 1) * nx + j);
      rowptr.push_back((int32_t)colidx.size());
    }
  std::vector<int32_t> agg(n);
  const int caps[] = {1, 4, 32, n, n + 7};
  for (int cap : caps) {
    const int count = ipx_aggregate_greedy(n, rowptr.data(), colidx.data(), cap, agg.data());
    const int bad = count < 1 ? 3 : check(agg, count, cap);
    if (bad || (cap == 1 && count != n) || (cap >= n && count != 1)) {
      printf("grid, cap %d: count %d, check %d\n", cap, count, bad);
      return 1;
    }
  }
  // rows without neighbours (an empty row, a row with its diagonal only)
  const int32_t rp2[] = {0, 0, 1, 3, 5};
  const int32_t ci2[] = {1, 2, 3, 2, 3};
  std::vector<int32_t> agg2(4);
  if (ipx_aggregate_greedy(4, rp2, ci2, 32, agg2.data()) != 3 || check(agg2, 3, 32) ||
      agg2[2] != agg2[3]) {
    printf("isolated rows\n");
    return 1;
  }
  const int32_t rp0[] = {0};
  if (ipx_aggregate_greedy(0, rp0, nullptr, 32, agg2.data()) != 0) return 1;
  // refused: cap < 1, a column out of range
  const int32_t bad_ci[] = {1, 2, 3, 2, 4};
  if (ipx_aggregate_greedy(4, rp2, ci2, 0, agg2.data()) >= 0 ||
      ipx_aggregate_greedy(4, rp2, bad_ci, 32, agg2.data()) >= 0) {
    printf("bad arguments accepted\n");
    return 1;
  }
  printf("aggregate ok\n");
  return 0;
}
