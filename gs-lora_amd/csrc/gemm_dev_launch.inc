// gemm_dev_launch.inc — development build only (-DGSL_DEV; included by gemm.hip in front of launch_op16): the lab's share of the 16-bit GEMM launch.
// launch_op16 calls dev_launch() once, before the product rule. It returns true when a lab kernel took the call (rc = its launch status);
// otherwise `tile` holds the product tile to run, which GSL_GEMM_VARIANT / GSL_GELU_VARIANT may have changed. Knobs (all read per launch):
//   GSL_GEMM_VARIANT   plain form: 1 / 3 / 8 / 12 force a product kernel (128x128 single stage, 256x128 three-stage ring, 256x256 8-phase, the 64-row
//                      ring kernel in the form small_ring_tile picks); 4 (256x256 two-stage), 9 (256x128x32, two workgroups per CU; GSL_STAGGER),
//                      10 (persistent ping-pong; GSL_PP_ABL), 11 (in-wave pipelined; GSL_PP_ABL), 13-15 (ring3w probes) are lab kernels. A value
//                      that names no kernel for the epilogue runs the 128x128 kernel. In-kernel-LoRA form: 4 = the single-phase 256x256 kernel.
//   GSL_GELU_VARIANT   the same for BIAS_GELU calls that the rule puts on the 8-phase kernel (without GSL_GEMM_VARIANT)
//   GSL_GEMM_ABL       main-loop ablation of the 256x128 ring kernel, plain STORE (tools/bench_gemm_abl.py)
//   GSL_W4, GSL_O4 / GSL_O4_ONE_PER_CU   the 4-wave kernel (gemm_w4.inc) / the overlap kernel (gemm_o4.inc) in place of the 8-phase kernel where
//                      their shape rules hold
//   -DGSL_P8_PERSISTENT=1 builds: the persistent form of the 8-phase kernel for plain stores with at least two rounds of tiles (gemm_dev_c.inc)
#if GSL_P8_PERSISTENT
// workgroups of the persistent kernels: one per CU
static inline int p8p_grid() {
  int n = num_cus();
  n -= n % 8;      // xcd_remap of the sequence numbers assumes seq % 8 = blockIdx % 8
  return n < 8 ? 8 : n;
}
#endif

template <int EPI, bool LORA>
static bool dev_launch(const GemmCall& c, int& tile, int& rc) {
  const EpiArgs& e = c.e;
  const int K1 = c.K1, K2 = c.K2;
  const bf16_t *A1 = (const bf16_t*)c.A1, *W1 = (const bf16_t*)c.W1, *A2 = (const bf16_t*)c.A2, *W2 = (const bf16_t*)c.W2;
  const char* ev = getenv("GSL_GEMM_VARIANT");
  auto tiles = [&](int bm, int bn) { return ((e.M + bm - 1) / bm) * ((e.N + bn - 1) / bn); };
  auto took = [&](const char* what) { rc = check_launch(what); return true; };
  if constexpr (LORA) {
    if (ev && atoi(ev) == 4) {
      hipLaunchKernelGGL(gemm_bf16_t256_lora_kernel<EPI>, dim3(tiles(BM4, BN4)), dim3(512), 0, c.st, A1, c.lda1, W1, c.ldw1, K1, c.lk, e);
      return took("gsl_gemm_nt_lora");
    }
    return false;
  } else {
    // the tile rule as the variant numbers the knobs speak
    int variant = tile == GSL_TILE_P8 ? 8 : tile == GSL_TILE_RING256X128 ? 3 : tile == GSL_TILE_128 ? 1 : 12;
    if (ev) variant = atoi(ev);
    if (EPI == GSL_EPI_BIAS_GELU && !ev && variant == 8) { const char* gv = getenv("GSL_GELU_VARIANT"); if (gv) variant = atoi(gv); }
    // kernels with the argument list of the ring / single-stage kernels
    auto launch = [&](auto kernel, int nb, int nt, const EpiArgs& ek) {
      hipLaunchKernelGGL(kernel, dim3(nb), dim3(nt), 0, c.st, A1, c.lda1, W1, c.ldw1, K1, A2, c.lda2, W2, c.ldw2, K2, ek);
    };
    if constexpr (EPI == GSL_EPI_STORE || EPI == GSL_EPI_BIAS_GELU) {
      const bool pp = variant == 10 && (K1 + K2) >= 192 && (e.N % 8) == 0 && (e.ldo % 8) == 0 && e.N >= 8;
      const bool iw = variant == 11 && (e.M % IW_TM) == 0 && (e.N % IW_TN) == 0 && (e.ldo % 8) == 0 && (K1 % 64) == 0 && (K2 % 64) == 0 &&
                      ((K1 + K2) == 512 || (K1 + K2) == 576) && (EPI != GSL_EPI_BIAS_GELU || e.out2);
      if (pp || iw) {
        EpiArgs ea = e;
        { const char* ab = getenv("GSL_PP_ABL"); ea.T = ab ? atoi(ab) : 0; }
        const int ntm = pp ? (e.M + PP_TM - 1) / PP_TM : e.M / IW_TM, ntn = pp ? (e.N + PP_TN - 1) / PP_TN : e.N / IW_TN;
        const int nunits = ntm * ((ntn % 2 == 0) ? 2 : 1);
        const int grid = nunits < 256 ? nunits : 256;
        if (pp) { launch(gemm_bf16_pp_kernel<EPI>, grid, 512, ea); return took("gsl_gemm_nt(pp)"); }
        if ((K1 + K2) == 576) launch(gemm_bf16_iw_kernel<EPI, 9>, grid, 512, ea);
        else launch(gemm_bf16_iw_kernel<EPI, 8>, grid, 512, ea);
        return took("gsl_gemm_nt(iw)");
      }
    }
    if constexpr (EPI != GSL_EPI_BIAS_RES_BF16 && EPI != GSL_EPI_PATCH_BF16 && EPI != GSL_EPI_MUL_G8 && EPI != GSL_EPI_BIAS_GELU_G8) {
      if (variant == 9) {
        EpiArgs e9 = e;
        if (EPI != GSL_EPI_PATCH) { const char* sg = getenv("GSL_STAGGER"); e9.T = sg ? atoi(sg) : 0; }
        launch(gemm_bf16_k32x2_kernel<EPI>, tiles(256, 128), 512, e9);
        return took("gsl_gemm_nt(k32x2)");
      }
      if (variant == 4) {
        launch(gemm_bf16_t256_kernel<EPI>, tiles(BM4, BN4), 512, e);
        return took("gsl_gemm_nt(t256)");
      }
    }
    if constexpr (EPI == GSL_EPI_STORE) {
      // probe: W fragments straight from L2 into registers (13 full, 14 A-DMA stream alone, 15 A-DMA + W loads alone)
      if (variant >= 13 && variant <= 15) {
        if (variant == 13) launch(gemm_bf16_ring3w_kernel<EPI, 0>, tiles(BM3, BN3), 512, e);
        else if (variant == 14) launch(gemm_bf16_ring3w_kernel<EPI, 1>, tiles(BM3, BN3), 512, e);
        else launch(gemm_bf16_ring3w_kernel<EPI, 2>, tiles(BM3, BN3), 512, e);
        return took("gsl_gemm_nt(ring3w probe)");
      }
      const char* ab = getenv("GSL_GEMM_ABL");
      const int abl = ab ? atoi(ab) : 0;
      if (variant == 3 && abl) {
        const int nb3 = tiles(BM3, BN3);
        switch (abl) {
          case 1: launch(gemm_bf16_ring3_kernel<EPI, 1>, nb3, 512, e); break;
          case 2: launch(gemm_bf16_ring3_kernel<EPI, 2>, nb3, 512, e); break;
          case 3: launch(gemm_bf16_ring3_kernel<EPI, 3>, nb3, 512, e); break;
          case 4: launch(gemm_bf16_ring3_kernel<EPI, 4>, nb3, 512, e); break;
          case 5: launch(gemm_bf16_ring3_kernel<EPI, 5>, nb3, 512, e); break;
          case 6: launch(gemm_bf16_ring3_kernel<EPI, 6>, nb3, 512, e); break;
          case 9: launch(gemm_bf16_ring3_kernel<EPI, 9>, nb3, 512, e); break;
          default: launch(gemm_bf16_ring3_kernel<EPI, 11>, nb3, 512, e);
        }
        return took("gsl_gemm_nt(ring3 ablation)");
      }
#if GSL_P8_PERSISTENT
      // plain-store GEMMs (QKV, out-proj dX, QKV dX, LoRA-free dX) with at least two rounds of tiles: the persistent form (see the kernel)
      const int nt8 = tiles(BM4, BN4);
      if (variant == 8 && (e.N % 8) == 0 && (e.ldo % 8) == 0 && nt8 >= 2 * p8p_grid()) {
        hipLaunchKernelGGL((gemm_bf16_p8p_kernel<EPI>), dim3(p8p_grid()), dim3(512), 0, c.st, A1, c.lda1, W1, c.ldw1, K1, A2, c.lda2, W2, c.ldw2, K2, nt8, e);
        return took("gsl_gemm_nt(p8p)");
      }
#endif
      // GSL_W4=1: plain-store GEMMs on the 4-wave 32x32x16 kernel where its shape rules hold (gemm_w4.inc; measured alternative)
      const char* w = getenv("GSL_W4");
      if (w && atoi(w) == 1 && variant == 8 && w4_usable(e.M, e.N, K1, K2, c.lda1, c.ldw1, e.ldo)) {
        hipLaunchKernelGGL((gemm_op16_w4_kernel<EPI>), dim3(((e.M + 255) / 256) * (e.N / 256)), dim3(256), 0, c.st, (const op16_t*)A1, c.lda1,
                           (const op16_t*)W1, c.ldw1, K1, e);
        return took("gsl_gemm_nt(w4)");
      }
    }
    if constexpr (EPI == GSL_EPI_STORE || EPI == GSL_EPI_BIAS_GELU_G8) {
      // GSL_O4=1: the plain-store and fused-FFN1 GEMMs of the 8-phase class on the overlap kernel where its shape rules hold (gemm_o4.inc; a
      // measured alternative). GSL_O4_ONE_PER_CU=1: 16 KB of dynamic LDS on top = one workgroup per CU.
      const char* o = getenv("GSL_O4");
      if (o && atoi(o) != 0 && variant == 8 && !(EPI == GSL_EPI_STORE && e.out2) && o4_usable(e.M, e.N, K1, K2, c.lda1, c.ldw1, c.lda2, c.ldw2, e.ldo)) {
        const char* o1 = getenv("GSL_O4_ONE_PER_CU");
        const int o4_dyn = (o1 && atoi(o1)) ? 16384 : 0;
        hipLaunchKernelGGL((gemm_op16_o4_kernel<EPI>), dim3(((e.M + O4_BM - 1) / O4_BM) * (e.N / O4_BN)), dim3(256), o4_dyn, c.st, (const op16_t*)A1,
                           c.lda1, (const op16_t*)W1, c.ldw1, K1, (const op16_t*)A2, c.lda2, (const op16_t*)W2, c.ldw2, K2, e);
        return took("gsl_gemm_nt(o4)");
      }
    }
    // no lab kernel: the product kernel the knob names (none of 3 / 8 / 12: the 128x128 kernel)
    tile = variant == 8 ? GSL_TILE_P8 : variant == 3 ? GSL_TILE_RING256X128 : variant == 12 ? small_ring_tile(e.M, e.N, K1 + K2) : GSL_TILE_128;
    return false;
  }
}
