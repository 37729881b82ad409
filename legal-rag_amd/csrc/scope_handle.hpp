// The scope handle (amdr_scope_t) as the files that stage through it see it: scope.hip (the scoped channel searches) and
// facet.hip (the host twin of the facet counts).  A workspace holder: it owns no table.
#pragma once
#include "common.hpp"

#include <mutex>

struct amdr_scope {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex mu;
  // the reserve of the "_device" calls: its sizes and the byte offset / length of each channel's region in ws[0]
  int nq_max = 0, k_max = 0;
  int64_t rows_max = 0;
  size_t off[3] = {0, 0, 0}, len[3] = {0, 0, 0};
  amdr::DevBuf ws[2];  // [0]: "_device" calls, [1]: host-pointer calls (see dense.hip)
  amdr::DevBuf stage;  // host-pointer calls: the table, the query operand and the result lists
};
