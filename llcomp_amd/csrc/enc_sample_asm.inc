// enc_sample_asm.inc -- the body of the hand-written encoder sample, included twice by enc_rows_asm.hpp:
//   LL_SNAP == 0  enc_rows_sample_asm: the eight states come from (and go back to) an LDS row bank -- the 1-row-slice kernels;
//   LL_SNAP == 1  enc_snap_sample_asm: the eight states arrive in two registers and are NOT written back -- the 2-D encoder, whose
//                 states were replayed ahead of it (snapshot_kernels.hip): LL_STATE(...) drops every state access.
// No include guard on purpose.
#if LL_SNAP
#define LL_STATE(...)
#else
#define LL_STATE(...) __VA_ARGS__
#endif
// one bin of the nested unary prefix on slot K (1..3): the lanes in exec code "ex > K-1"; those with a 1 stay
#define LL_UNARY(K, KM1, EL, EH, N, SAVE)                  \
    LL_SPLIT(EL)                                           \
    LL_STATE("ds_write_b8 %[bank], " EL " offset:" K "\n\t") \
    LL_NARROW("lt_u32", KM1, LL_EX)                        \
    SAVE                                                   \
    "s_cbranch_execz .Lunary_done_%=\n\t"                  \
    LL_ONE                                                 \
    LL_STATE("ds_write_b8 %[bank], " EH " offset:" K "\n\t") \
    LL_RENORM(N)
// Codes residual `res` in the context whose 8 state bytes sit at LDS address `bank`; low_range = RangeEnc::low | ::range << 32,
// wp as in RangeEnc (slice_kernels.hip; all LDS addresses are byte addresses), `base` = LDS address of the lane's staging area (carries walk
// back to it).
#if LL_SNAP
__device__ __forceinline__ void enc_snap_sample_asm(unsigned long long& low_range, uint32_t& wp, EncRowsExtra& x, uint32_t b0, uint32_t b1,
                                                    int res, uint32_t base) {
#else
__device__ __forceinline__ void enc_rows_sample_asm(unsigned long long& low_range, uint32_t& wp, EncRowsExtra& x, uint32_t bank,
                                                    int res, uint32_t base) {
#endif
    asm volatile(
        "s_mov_b64 " LL_SX ", exec\n\t"
        LL_STATE("ds_read2st64_b32 " LL_B ", %[bank] offset1:1\n\t")
        "s_cmp_lg_u32 %[hot], 0\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"  // (both forms: the lgkmcnt(7) below counts exactly this block's eight reads -- nothing of hipcc's may still be in flight)
        "v_lshlrev_b32_sdwa " LL_E0L ", " LL_C3 ", " LL_B0 " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0\n\t"
        "ds_read_b64 " LL_E0 ", " LL_E0L "\n\t"
        "s_cbranch_scc0 .Lcold_%=\n\t"
        LL_FETCH_REST
        "s_waitcnt lgkmcnt(7)\n\t"
        "s_branch .Lzero_%=\n"
        ".Lcold_%=:\n\t"
        "s_waitcnt lgkmcnt(0)\n"
        // ---- slot 0: "the residual is zero" (a 1 for the lanes whose residual IS zero)
        ".Lzero_%=:\n\t"
        LL_SPLIT(LL_E0L)
        LL_STATE("ds_write_b8 %[bank], " LL_E0L "\n\t")
        "v_cmp_eq_u32_e32 vcc, 0, %[res]\n\t"
        "s_andn2_b64 " LL_SA ", exec, vcc\n\t"  // the lanes with a non-zero residual
        "s_and_saveexec_b64 " LL_ST ", vcc\n\t"
        LL_PATCH_SKIP("0")
        LL_ONE
        LL_STATE("ds_write_b8 %[bank], " LL_E0H "\n")
        LL_PATCH_END("0")
        LL_RENORM("0")
        "s_and_b64 exec, " LL_SA ", " LL_SA "\n\t"
        "s_cbranch_execz .Ldone_%=\n\t"
        "s_mov_b64 " LL_SB ", 0\n\t"  // (slot 1 may not be reached by anybody: nobody codes slot 5 then)
        "s_mov_b64 " LL_SM ", 0\n\t"
        "s_cmp_lg_u32 %[hot], 0\n\t"
        "s_cbranch_scc1 .Lhave_%=\n\t"
        LL_FETCH_REST
        ".Lhave_%=:\n\t"
        "v_sub_u32_e32 " LL_A ", 0, %[res]\n\t"
        "v_max_i32_e32 " LL_A ", %[res], " LL_A "\n\t"
        "v_ffbh_u32_e32 " LL_EX ", " LL_A "\n\t"
        "v_sub_u32_e32 " LL_EX ", 31, " LL_EX "\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        // ---- unary exponent: slots 1, 2, 3 once each, then a run on slot 4; exec only shrinks until .Lunary_done
        // (the lane sets of slots 2 and 3 are the lane sets of slot 5 and of the mantissa run: kept, not compared for again)
        LL_UNARY("1", "0", LL_E1L, LL_E1H, "1", "s_mov_b64 " LL_SB ", exec\n\t")
        LL_UNARY("2", "1", LL_E2L, LL_E2H, "2", "s_mov_b64 " LL_SM ", exec\n\t")
        LL_UNARY("3", "2", LL_E3L, LL_E3H, "3", "")
        "s_mov_b64 " LL_SU ", exec\n\t"
        "v_add_u32_e32 " LL_N ", -3, " LL_EX "\n\t"
        "s_mov_b32 " LL_SI ", 0\n\t"
        // (both run loops are tested at the bottom: the first test stands in front, the back edge is the exit test's own branch)
        LL_SPLIT(LL_E4L)
        LL_NARROW("lt_u32", LL_SI, LL_N)
        "s_cbranch_execz .Ltail_done_%=\n\t"
        ".p2align 6\n"  // (the two run loops start on a 64-byte line of the instruction cache)
        ".Ltail_%=:\n\t"
        "v_lshrrev_b32_e32 " LL_OFF ", 16, " LL_E4H "\n\t"
        "ds_read_b64 " LL_E4 ", " LL_OFF "\n\t"
        LL_ONE
        LL_RENORM("4")
        "s_add_i32 " LL_SI ", " LL_SI ", 1\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        LL_SPLIT(LL_E4L)
        LL_NARROW("lt_u32", LL_SI, LL_N)
        "s_cbranch_execnz .Ltail_%=\n"
        ".Ltail_done_%=:\n\t"
        "s_mov_b64 exec, " LL_SU "\n\t"
        LL_STATE("ds_write_b8 %[bank], " LL_E4L " offset:256\n")
        ".Lunary_done_%=:\n\t"
        "s_mov_b64 exec, " LL_SA "\n\t"
        LL_RENORM("5")  // of the lanes whose last unary bin was the closing zero
        // ---- slot 5: the mantissa bit below the leading one, then the rest of the mantissa as a run on slot 6
        "s_and_b64 exec, " LL_SB ", " LL_SB "\n\t"  // the lanes with an exponent > 0
        "s_cbranch_execz .Lsign_%=\n\t"
        LL_SPLIT(LL_E5L)
        LL_STATE("ds_write_b8 %[bank], " LL_E5L " offset:257\n\t")
        "v_lshl_or_b32 " LL_BITS ", " LL_A ", 1, 1\n\t"
        "v_sub_u32_e32 " LL_T ", 31, " LL_EX "\n\t"
        "v_lshlrev_b32_e32 " LL_BITS ", " LL_T ", " LL_BITS "\n\t"
        "v_add_co_u32_e32 " LL_BITS ", vcc, " LL_BITS ", " LL_BITS "\n\t"
        "s_and_saveexec_b64 " LL_ST ", vcc\n\t"
        LL_PATCH_SKIP("5")
        LL_ONE
        LL_STATE("ds_write_b8 %[bank], " LL_E5H " offset:257\n")
        LL_PATCH_END("5")
        LL_RENORM("6")
        LL_NARROW("ne_u32", "%[sent]", LL_BITS)
        "s_cbranch_execz .Lman_done_%=\n\t"
        ".p2align 6\n"
        ".Lman_%=:\n\t"
        "v_add_co_u32_e32 " LL_BITS ", vcc, " LL_BITS ", " LL_BITS "\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        LL_SPLIT(LL_E6L)
        "v_lshrrev_b32_e32 " LL_OFF ", 16, " LL_E6L "\n\t"
        "s_and_saveexec_b64 " LL_ST ", vcc\n\t"
        LL_PATCH_SKIP("6")
        LL_ONE
        "v_lshrrev_b32_e32 " LL_OFF ", 16, " LL_E6H "\n"
        LL_PATCH_END("6")
        "ds_read_b64 " LL_E6 ", " LL_OFF "\n\t"
        LL_RENORM("7")
        LL_NARROW("ne_u32", "%[sent]", LL_BITS)
        "s_cbranch_execnz .Lman_%=\n\t"
        "s_branch .Lman_done_%=\n"  // (once per sample, over the out-of-line part)
        // ---- out of line: the carry subroutine and its call stubs
        LL_RARE_STUB("0") LL_RARE_STUB("1") LL_RARE_STUB("2") LL_RARE_STUB("3") LL_RARE_STUB("4")
        LL_RARE_STUB("5") LL_RARE_STUB("6") LL_RARE_STUB("7") LL_RARE_STUB("8")
        // exec = the lanes that renormalise, vcc = those of them whose held 0xFF took a carry: +1 into the bytes before the
        // one just stored (llcomp.hpp:40-57 resolved eagerly), walking back through the staging area; what would go on
        // below it (bytes already in HBM) is left to the caller: `pend`.
        ".Lcarry_%=:\n\t"
        "s_and_saveexec_b64 " LL_SC ", vcc\n\t"
        "v_add_u32_e32 " LL_CK ", -1, %[wp]\n"
        ".Lcloop_%=:\n\t"
        "v_cmp_lt_u32_e32 vcc, " LL_CK ", %[base]\n\t"
        "s_and_b64 " LL_SD ", exec, vcc\n\t"
        "s_cbranch_scc0 .Lcin_%=\n\t"
        "s_mov_b64 " LL_SE ", exec\n\t"
        "s_mov_b64 exec, " LL_SD "\n\t"
        "v_mov_b32_e32 %[pend], 1\n\t"
        "s_mov_b32 %[anyp], 1\n\t"
        "s_andn2_b64 exec, " LL_SE ", " LL_SD "\n\t"
        "s_cbranch_execz .Lcdone_%=\n"
        ".Lcin_%=:\n\t"
        "ds_read_u8 " LL_CT ", " LL_CK "\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_add_u32_e32 " LL_CT2 ", 1, " LL_CT "\n\t"
        "ds_write_b8 " LL_CK ", " LL_CT2 "\n\t"
        "v_add_u32_e32 " LL_CK ", -1, " LL_CK "\n\t"
        "v_cmp_eq_u32_e32 vcc, 0xff, " LL_CT "\n\t"
        "s_and_b64 exec, exec, vcc\n\t"
        "s_cbranch_execnz .Lcloop_%=\n"
        ".Lcdone_%=:\n\t"
        "s_mov_b64 exec, " LL_SC "\n\t"
        "v_and_b32_e32 " LL_LOW ", 0xffffff, " LL_LOW "\n\t"  // the carry is spent (it must not reach `range` in the 64-bit shift)
        "s_add_u32 " LL_SRL ", " LL_SRL ", 4\n\t"
        "s_addc_u32 " LL_SRH ", " LL_SRH ", 0\n\t"
        "s_setpc_b64 " LL_SR "\n"
        // ---- back in line
        ".Lman_done_%=:\n\t"
        "s_mov_b64 exec, " LL_SM "\n\t"  // the lanes with an exponent > 1: those that ran
        LL_STATE("v_lshrrev_b32_e32 " LL_T ", 3, " LL_OFF "\n\t")
        LL_STATE("ds_write_b8 %[bank], " LL_T " offset:258\n")
        // ---- slot 7: the sign
        ".Lsign_%=:\n\t"
        "s_mov_b64 exec, " LL_SA "\n\t"
        LL_SPLIT(LL_E7L)
        LL_STATE("ds_write_b8 %[bank], " LL_E7L " offset:259\n\t")
        "v_cmp_gt_i32_e32 vcc, 0, %[res]\n\t"
        "s_and_saveexec_b64 " LL_ST ", vcc\n\t"
        LL_PATCH_SKIP("7")
        LL_ONE
        LL_STATE("ds_write_b8 %[bank], " LL_E7H " offset:259\n")
        LL_PATCH_END("7")
        LL_RENORM("8")
        ".Ldone_%=:\n\t"
        "s_bcnt1_i32_b64 " LL_S1 ", " LL_SA "\n\t"
        "s_bcnt1_i32_b64 " LL_S2 ", " LL_SX "\n\t"
        "s_lshl_b32 " LL_S1 ", " LL_S1 ", 1\n\t"
        "s_cmp_ge_u32 " LL_S1 ", " LL_S2 "\n\t"
        "s_cselect_b32 %[hot], 1, 0\n\t"
        "s_mov_b64 exec, " LL_SX "\n\t"
#if LL_SNAP
        : "+{v[30:31]}"(low_range), [wp] "+v"(wp), [pend] "+v"(x.pend), [hot] "+s"(x.hot), [anyp] "+s"(x.any_pend), "+{v32}"(b0), "+{v33}"(b1)
        : [res] "v"(res),
#else
        : "+{v[30:31]}"(low_range), [wp] "+v"(wp), [pend] "+v"(x.pend), [hot] "+s"(x.hot), [anyp] "+s"(x.any_pend)
        : [bank] "v"(bank), [res] "v"(res),
#endif
          [base] "v"(base), [c100] "s"(0x100u), [cwrap] "s"(0xFFFFFFu),
          [sent] "s"(0x80000000u), [c3] "v"(3u)
        : "vcc", "scc", "memory",
#if !LL_SNAP
          "v32", "v33",
#endif
          "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44",
          "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43",
          "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s56", "s57");
}


#undef LL_STATE
#undef LL_UNARY
