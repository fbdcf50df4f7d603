// What lineconv.hip shares with colconv.hip.
#pragma once

#include <ATen/ATen.h>

namespace dtmx {

// wp[c][T-1-t][ko] = w[ko][t][c] (the dgrad operand of a 1xT / Tx1 weight:
// taps reversed, each tap transposed), one launch on the current stream.
// w is [Ko][T][C] at element alignment, wp a dense [C][T][Ko] allocation.
void lineconv_pack(const at::Tensor& w, at::Tensor& wp, long C, long Ko, long T);

}  // namespace dtmx
