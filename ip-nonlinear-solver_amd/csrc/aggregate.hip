// Greedy aggregation of the graph of S = A A' for the aggregate blocks and the coarse level of
// the preconditioned CG (ipsolver/iterative.py; csrc/pcg.hip).  Host code only: no device calls.
#include <stdint.h>
#include <vector>
#include "../../include/ipx.h"

extern "C" {

// Seeds s = 0, 1, ... in index order, assigned rows skipped.  A new aggregate starts as [s]; its
// member list is walked from the head and, for each member, its neighbours in the column order
// of its row of S: every unassigned one is appended and assigned at once while the aggregate has
// fewer than `cap` members.  Aggregates are therefore connected in S and not empty.
int ipx_aggregate_greedy(int64_t n, const int32_t *rowptr, const int32_t *colidx, int32_t cap,
                         int32_t *agg) {
  if (n < 0 || n > INT32_MAX || cap < 1 || !rowptr || !agg) return IPX_EINVAL;
  if (n > 0 && rowptr[n] > 0 && !colidx) return IPX_EINVAL;
  for (int64_t i = 0; i < n; ++i) agg[i] = -1;
  std::vector<int32_t> members((size_t)cap);
  int32_t count = 0;
  for (int32_t s = 0; s < (int32_t)n; ++s) {
    if (agg[s] >= 0) continue;
    int32_t len = 0;
    members[len++] = s;
    agg[s] = count;
    for (int32_t head = 0; head < len && len < cap; ++head) {
      const int32_t i = members[head];
      for (int32_t p = rowptr[i]; p < rowptr[i + 1] && len < cap; ++p) {
        const int32_t j = colidx[p];
        if (j < 0 || j >= n) return IPX_EINVAL;
        if (agg[j] < 0) {
          agg[j] = count;
          members[len++] = j;
        }
      }
    }
    ++count;
  }
  return count;
}

}  // extern "C"
