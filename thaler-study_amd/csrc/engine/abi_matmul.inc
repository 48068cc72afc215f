// Part of sumcheck_hip.hip (included there, in order): C ABI: the matrix product C = A * B (kernels/matmul.hpp).

// =====================================================================================
// C ABI: sc_matmul - step 1 of the MatMult protocol (the reference's tests form `Matrix * Matrix` and prove it)
// =====================================================================================

namespace {

// which kernel computes the product: 1 int8 matrix cores, 2 VALU tiles, 3 VALU one thread per entry (the launch log's kf)
int matmul_kernel_of(const sc_ctx* ctx, size_t n) {
  if (ctx->matmul_path == 1 && n >= 4) return 1;
  if (ctx->matmul_path == 0 && n >= 5) return 1;
  return n >= 6 ? 2 : 3;
}

int matmul_impl(sc_ctx* ctx, const u64* A, const u64* B, size_t n, u64* C) {
  const size_t N = (size_t)1 << n, len = N * N;
  const int k = (int)n;
  const int which = matmul_kernel_of(ctx, n);
  if (which == 1) {
    // scratch: A8 | B8t (eight byte planes each, rows padded to KP) | SA | SB (eight u32 sums per row / column)
    const size_t KP = std::max<size_t>(N, sc::kMatmulStepK), plane = N * KP;
    const size_t bytes = 16 * plane + 2 * 8 * N * sizeof(unsigned);
    PoolBuf scratch;   // (given back on return: stream-ordered reuse)
    SC_TRY(scratch.alloc(ctx, (bytes + 7) / 8));
    unsigned char* a8 = reinterpret_cast<unsigned char*>(scratch.get());
    unsigned char* b8t = a8 + 8 * plane;
    unsigned* sa = reinterpret_cast<unsigned*>(b8t + 8 * plane);
    unsigned* sb = sa + 8 * N;
    if (hipMemsetAsync(sa, 0, 2 * 8 * N * sizeof(unsigned), ctx->stream) != hipSuccess) return fail(ctx, SC_ERR_HIP, "sc_matmul: memset failed");
    // repack: reads both matrices, writes the planes and the sums
    SC_TRY(timer_begin(ctx, SC_KIND_MATMUL, 0, k, 2 * k, (u64)16 * len, (u64)16 * plane + 64 * N));
    {
      const size_t a_threads = N * (KP / 16), b_threads = N * (KP / std::min<size_t>(KP, sc::kMatmulBRun));
      const unsigned a_grid = (unsigned)std::min<size_t>((a_threads + sc::kBlock - 1) / sc::kBlock, (size_t)8 * ctx->num_cus);
      const unsigned b_grid = (unsigned)std::min<size_t>((b_threads + sc::kBlock - 1) / sc::kBlock, (size_t)8 * ctx->num_cus);
      SC_DISPATCH_FIELD(ctx, F, f, {
        hipLaunchKernelGGL((sc::matmul_bytes_a_kernel<F>), dim3(a_grid), dim3(sc::kBlock), 0, ctx->stream, f, A, k, KP, a8, sa);
        hipLaunchKernelGGL((sc::matmul_bytes_b_kernel<F>), dim3(b_grid), dim3(sc::kBlock), 0, ctx->stream, f, B, k, KP, b8t, sb);
      });
      if (hipGetLastError() != hipSuccess) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "matmul_bytes kernel launch failed");
      }
      SC_TRY(timer_end(ctx));
    }
    // product: every plane byte once, C once
    SC_TRY(timer_begin(ctx, SC_KIND_MATMUL, 1, k, 2 * k, (u64)16 * plane + 64 * N, (u64)8 * len));
    {
      const size_t waves = (N / 16) * (N / 16);
      const unsigned grid = (unsigned)std::min<size_t>((waves + 3) / 4, (size_t)8 * ctx->num_cus);
      SC_DISPATCH_FIELD(ctx, F, f,
                        hipLaunchKernelGGL((sc::matmul_mfma_kernel<F>), dim3(grid), dim3(sc::kBlock), 0, ctx->stream, f,
                                           (const unsigned char*)a8, (const unsigned char*)b8t, (const unsigned*)sa, (const unsigned*)sb, k, KP, C));
      if (hipGetLastError() != hipSuccess) {
        poison(ctx);
        return fail(ctx, SC_ERR_HIP, "matmul_mfma_kernel launch failed");
      }
    }
    return timer_end(ctx);
  }
  SC_TRY(timer_begin(ctx, SC_KIND_MATMUL, which, k, 2 * k, (u64)16 * len, (u64)8 * len));
  SC_DISPATCH_FIELD(ctx, F, f, {
    if (which == 2)
      hipLaunchKernelGGL((sc::matmul_tiled_kernel<F>), dim3((unsigned)std::min<size_t>((N / 64) * (N / 64), (size_t)4 * ctx->num_cus)),
                         dim3(sc::kBlock), 0, ctx->stream, f, A, B, k, C);
    else
      hipLaunchKernelGGL((sc::matmul_kernel<F>), dim3(grid_for_wide(ctx, len)), dim3(sc::kBlock), 0, ctx->stream, f, A, B, k, C);
  });
  if (hipGetLastError() != hipSuccess) {
    poison(ctx);
    return fail(ctx, SC_ERR_HIP, "matmul kernel launch failed");
  }
  return timer_end(ctx);
}

}  // namespace

extern "C" int sc_matmul(sc_ctx* ctx, const sc_table* A, const sc_table* B, size_t n, sc_table** C) {
  if (!ctx || !C) return SC_ERR_ARG;
  *C = nullptr;
  if (is_multi(ctx) || ctx->world > 1)
    return fail(ctx, SC_ERR_UNSUPPORTED, "sc_matmul: products run on a context of one device and one rank (this one is %s)",
                is_multi(ctx) ? "a multi-device handle" : "sharded");
  SC_TRY(check_pair(ctx, A, B, "sc_matmul"));
  if (n > 14) return fail(ctx, SC_ERR_ARG, "sc_matmul: 2^%zu x 2^%zu matrices (at most 2^14 x 2^14)", n, n);
  if (A->len != ((size_t)1 << (2 * n))) return fail(ctx, SC_ERR_ARG, "sc_matmul: tables must have 2^(2n) = 2^%zu entries, not %zu", 2 * n, A->len);
  SC_TRY(set_device(ctx));
  TableBuf out;
  SC_TRY(out.alloc(ctx, A->len));
  SC_TRY(matmul_impl(ctx, A->d, B->d, n, out->d));
  *C = out.release();
  return SC_OK;
}
