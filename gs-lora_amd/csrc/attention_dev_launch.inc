// attention_dev_launch.inc — development build only (-DGSL_DEV; included by attention.hip in front of attn_launch): the lab's share of the attention launch.
// attn_launch calls attn_dev_launch() once, after the kernel rule. It overwrites the development parameters of the call record (abl, stamps, imap,
// the no-store bit of qkv_layout) and `kernel`, the product kernel to run; it returns true when the two-kernel backward — which only this build
// holds for T > 64 — took the call (rc = its launch status). The knobs act on the 16-bit kernels up to T = 224; all are read per launch:
//   GSL_ATTN_PERSISTENT=0       forward: one item per workgroup instead of the persistent kernel
//   GSL_ATTN_ABL                1 staging only, 2 no staging (forward and the two-kernel backward); 4 no output stores (the 512-thread FAST fused backward)
//   GSL_ATTN_BWD_SPLIT=1        the two-kernel backward (dQ, then dK / dV) at T > 64; GSL_ATTN_NT key tiles per wave of its dK / dV kernel (1 or 2;
//                               measured at B = 1024, T = 197: NT = 1, two workgroups per CU, 410 us, NT = 2 480 us)
//   GSL_ATTN_BWD_MERGED=0       the fused two-phase backward instead of the merged one; GSL_ATTN_BWD_MERGED_MIN items per CU from which the merged one runs (8)
//   GSL_ATTN_ITEM_REMAP=0       backward without the XCD item remap; GSL_ATTN_ITEM_REMAP_FWD=1 the persistent forward with it (B % 8 == 0, CUs % 8 == 0)
//   GSL_ATTN_STAMPS             device address of a cycle-stamp buffer (fused and merged backward)
static inline int attn_env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static inline unsigned long long* attn_stamps() { const char* sp = getenv("GSL_ATTN_STAMPS"); return sp ? reinterpret_cast<unsigned long long*>(strtoull(sp, nullptr, 0)) : nullptr; }

static bool attn_dev_launch(AttnCall& c, int dir, int& kernel, int& rc) {
  if (c.dtype != GSL_OP16 || c.T > 224 || (dir != ATTN_FWD && dir != ATTN_BWD)) return false;
  const int cus = num_cus();
  c.abl = attn_env("GSL_ATTN_ABL", 0);
  if (dir == ATTN_FWD) {
    c.imap = (c.B % 8 == 0 && cus % 8 == 0) ? attn_env("GSL_ATTN_ITEM_REMAP_FWD", 0) : 0;
    if (kernel == GSL_ATTN_FWD_PERSISTENT && !attn_env("GSL_ATTN_PERSISTENT", 1)) kernel = GSL_ATTN_FWD_512;      // (the rule's next row: items >= 2 CUs)
    return false;
  }
  if (c.T <= 64) return false;
  if (attn_env("GSL_ATTN_BWD_SPLIT", 0)) {
    const bf16_t *qkv = (const bf16_t*)c.qkv, *o = (const bf16_t*)c.o, *d_o = (const bf16_t*)c.d_o; bf16_t* out = (bf16_t*)c.out;
    const dim3 items(c.items), blk(512);
    hipLaunchKernelGGL(attn_bwd_dq_bf16_kernel<14>, items, blk, 0, c.st, qkv, o, d_o, c.lse, out, c.delta_ws, c.T, c.H, c.scale, c.abl, c.qkv_layout);
    auto dkv = attn_env("GSL_ATTN_NT", 1) == 1 ? attn_bwd_dkv_bf16_kernel<14, 1> : attn_bwd_dkv_bf16_kernel<14, 2>;
    hipLaunchKernelGGL(dkv, items, blk, 0, c.st, qkv, d_o, c.lse, c.delta_ws, out, c.T, c.H, c.scale, c.abl, c.qkv_layout);
    rc = check_launch("gsl_attention_bwd");
    return true;
  }
  c.stamps = attn_stamps();
  const bool merged = attn_fast(c.T) && c.items >= attn_env("GSL_ATTN_BWD_MERGED_MIN", 8) * cus && attn_env("GSL_ATTN_BWD_MERGED", 1);
  kernel = merged ? GSL_ATTN_BWD_MERGED : c.items < cus ? GSL_ATTN_BWD_FUSED_1024 : GSL_ATTN_BWD_FUSED_512;
  c.imap = attn_item_remap(c.B, cus, dir, kernel) ? attn_env("GSL_ATTN_ITEM_REMAP", 1) : 0;
  if (kernel == GSL_ATTN_BWD_FUSED_512 && attn_fast(c.T) && c.abl == 4) c.qkv_layout |= 2;      // the kernel's nostore bit
  return false;
}
