// What the row encoders of the Ligero-style commitment (ligero.hpp, expander.hpp) share: log2 of the codeword words a block takes -
// one codeword of 2^log_len words, or whole ones up to 2^kRowMinTileLog words (the matrix of 2^log_total words if that is less)
#pragma once

namespace sc {
constexpr int kRowMinTileLog = 12;
inline int row_tile_log(int log_len, int log_total) {
  return log_len >= kRowMinTileLog ? log_len : (log_total < kRowMinTileLog ? log_total : kRowMinTileLog);
}
}  // namespace sc
