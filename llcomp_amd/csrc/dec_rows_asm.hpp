// dec_rows_asm.hpp -- one sample of the decoder's FAST PATH for 1-row slices (getSymbol<true,4,6,7>, llcomp.hpp:219-247, over
// the range decoder, llcomp.hpp:98-121), hand-written for gfx950.  Same bins, same order, same arithmetic as
// dec_residual<*, false, true> in slice_kernels.hip, which documents the scheme and stays in use as the CHECKED replay (the block
// never looks at the fill level of the window: dec_sample rolls back and replays a sample that emptied it) and for the other
// kernel families.
//
// What the block does that hipcc's structurised code cannot (prices: tools/ubench/valu_rate3):
//   * the lane sets of the unary exponent are NESTED (the lanes that decode a 1 on slot k are the lanes that decode slot k + 1),
//     so exec only shrinks until the phase is over; every lane takes the outcome of a 0 IN PLACE (range = r0, low -= r0: a
//     borrow says the bin is a 0 and the lane drops out; `low` is put back and the refill done once behind the phase), where
//     the compiler keeps the difference apart and selects or copies per bin;
//   * the unary phase has TWO range registers that alternate (A = the outgoing range, B = LD_R1): a bin that reads its range from
//     one writes r1 straight into the other, under its own exec, and leaves r0 where it was -- no copy of r1 per bin.  A lane's r0
//     is then in A or in B by the parity of the bin it left on; the lanes that left on a B-bin are collected in one scalar mask
//     (LD_SB) and moved over once behind the phase.  r1 << 8 of a staying lane's refill is the product with its low byte masked
//     away (no left shift);
//   * `low` and the sample's private copy of the window's next three bytes are the two halves of ONE aligned register pair (low on
//     top, the copy's next byte in bits 31..24 below it): a refill is one v_lshlrev_b64 of the pair by 8;
//   * the mantissa run gathers its bits under a MARKER bit that the same add-with-carry pushes out as its carry when the lane's
//     last bit has come in: the carry is the loop's exit mask, no compare per bin;
//   * the "most lanes non-zero" flag is three scalar instructions on masks the block has anyway; no copies at merges; the two
//     run loops start on a 64-byte line of the instruction cache.
//
// LDS contract: the entries of the model table carry absolute LDS addresses of their successors (load_table); the row bank is
// the decoder's wide one (16-bit table addresses, [word 0..3][lane] 256 bytes apart, slot k in half k & 1 of word k / 2).
// Register contract: low, range and the window come in as READ-ONLY operands and leave as separate outputs (the block's first write
// of each goes to the output), so the inputs are still the state before the sample when the block is done: they are the rollback
// snapshot of the checked replay, nothing is saved per sample, and two consecutive samples can swap the roles of the two register
// sets without a copy between them.  The window pair is an ordinary operand too (its low half is passed a second time as a 32-bit
// operand: the block needs it by name).  The outgoing low : copy pair needs its halves by name as well, which an operand cannot
// give, so the block exists twice, on two fixed aligned pairs (SET 0: v[0:1], SET 1: v[2:3]); consecutive samples alternate,
// and the caller reads `low` as the pair's high half (no move: the incoming low of the next sample IS v1 / v3).
// The copy and its sentinel: the head forms it from the window's low dword by one v_perm_b32 -- stream byte 0 in bits 31..24, byte
// 1 in 23..16, byte 2 in 15..8, and 0xFF (the selector's constant) in bits 7..0.  Every refill shifts the pair up by 8, so behind
// the sample the lowest set bit of the copy stands at 0 / 8 / 16 / 24 = the bits the sample consumed (v_ffbl_b32, fed to the
// window's one 64-bit shift as it is).  A copy of 0 says: a fourth byte was wanted (it got the sentinel's 0xFF instead), or the
// block zeroed it for an exponent above 31 -- the caller replays that lane.
// The block owns v32..v45, v48..v52 and s56..s71 for its length, and the pair of its SET; with what hipcc needs around it the
// kernel stays below 64 VGPRs / 80 SGPRs (eight wavefronts per SIMD).  gfx950 hazards the assembler does not handle inside inline
// asm, checked by hand: a vector instruction that reads VCC follows the vector instruction that wrote it by two wait states (s_nop 1).
#pragma once
#include <cstdint>

namespace llcomp_mi {

#define LD_E0L "v32"
#define LD_E0H "v33"
#define LD_E0 "v[32:33]"
#define LD_E5L "v34"
#define LD_E5H "v35"
#define LD_E5 "v[34:35]"
#define LD_E6L "v36"
#define LD_E6H "v37"
#define LD_E6 "v[36:37]"
#define LD_E7L "v38"
#define LD_E7H "v39"
#define LD_E7 "v[38:39]"
#define LD_E1L "v40"
#define LD_E1H "v41"
#define LD_E1 "v[40:41]"
#define LD_E2L "v42"
#define LD_E2H "v43"
#define LD_E2 "v[42:43]"
#define LD_E3L "v44"
#define LD_E3H "v45"
#define LD_E3 "v[44:45]"
#define LD_E4L "v48"
#define LD_E4H "v49"
#define LD_E4 "v[48:49]"
#define LD_PROD "v50"  // range * P
#define LD_R1 "v51"    // range * P >> 8; the unary phase's second range register (B)
#define LD_DIFF "v52"  // low - r0
#define LD_OFF "v52"   // LDS address of a successor entry / of a fetched slot (never live together with the difference)
#define LD_EX "v32"    // exponent                         (slot 0 is over: its entry's registers are free)
#define LD_W "v33"     // mantissa bits gathered so far, inverted, under their leading one
#define LD_RUN "v40"   // mantissa run: marker + inverted bits   (slots 1..3 are over: their entries' registers are free)
#define LD_NX "v41"    //               half-entry the last bin chose
#define LD_T "v42"     // short-lived
#define LD_SX "s[56:57]"  // exec at entry
#define LD_SA "s[58:59]"  // lanes with a non-zero residual
#define LD_SW "s[60:61]"  // exec saved around a refill
#define LD_SP "s[62:63]"  // exec saved around a bit-1 patch; unary run: the lanes that leave on a B-bin
#define LD_S5 "s[64:65]"  // lanes that finish the sample (non-zero residual, valid exponent)
#define LD_SB "s[64:65]"  // unary phase: lanes whose r0 is in B (they left on slot 2 or on an odd bin of the run); shares LD_S5: read before it is set
#define LD_SU "s[66:67]"  // lanes of the run on slot 4; later: lanes that decode slot 5 (exponent > 0)
#define LD_SD "s[68:69]"  // mantissa run: lanes whose last bit has just come in
#define LD_S1L "s[68:69]"  // lanes with an exponent > 0 (the lanes that stayed behind slot 1); shares LD_SD: read before the run
#define LD_SM "s[70:71]"   // lanes with an exponent > 1; shares LD_S1 / LD_S2: read before the end
#define LD_S1 "s70"
#define LD_S2 "s71"

// r1 = range * P(entry) >> 8, range = r0 = range - r1: the outcome of a 0, in place
#define LD_SPLIT(EL)                                                                                                       \
    "v_mul_u32_u24_sdwa " LD_PROD ", " EL ", %[range] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
    "v_lshrrev_b32_e32 " LD_R1 ", 8, " LD_PROD "\n\t"                                                                      \
    "v_sub_u32_e32 %[range], %[range], " LD_R1 "\n\t"
// the same for the sample's first bin: reads the incoming range, writes the outgoing one
#define LD_SPLIT_IN(EL)                                                                                                       \
    "v_mul_u32_u24_sdwa " LD_PROD ", " EL ", %[range_in] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
    "v_lshrrev_b32_e32 " LD_R1 ", 8, " LD_PROD "\n\t"                                                                      \
    "v_sub_u32_e32 %[range], %[range_in], " LD_R1 "\n\t"
// the same for a bin of the unary phase: the range is in RD, r1 goes to WR (the other one of A / B), r0 stays in RD
#define LD_SPLIT_TO(EL, RD, WR)                                                                                       \
    "v_mul_u32_u24_sdwa " LD_PROD ", " EL ", " RD " dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD\n\t" \
    "v_lshrrev_b32_e32 " WR ", 8, " LD_PROD "\n\t"                                                                     \
    "v_sub_u32_e32 " RD ", " RD ", " WR "\n\t"
// a refill's byte: low = low << 8 | next byte of the sample's copy, which moves on
#define LD_TAKE "v_lshlrev_b64 " LD_PAIR ", 8, " LD_PAIR "\n"
// refill (llcomp.hpp:115-120) of the lanes in exec
#define LD_REFILL(N)                                         \
    "v_cmp_gt_u32_e32 vcc, %[c100], %[range]\n\t"            \
    "s_and_saveexec_b64 " LD_SW ", vcc\n\t"                  \
    "s_cbranch_execz .Lrf" N "_%=\n\t"                       \
    "v_lshlrev_b32_e32 %[range], 8, %[range]\n\t"            \
    LD_TAKE                                                  \
    ".Lrf" N "_%=:\n\t"                                      \
    "s_mov_b64 exec, " LD_SW "\n\t"
// the same for lanes that have just taken r1 (in WR) as their range: r1 << 8 = the product without its low byte
#define LD_REFILL_R1(WR, N)                                       \
    "v_cmp_gt_u32_e32 vcc, %[c100], " WR "\n\t"                   \
    "s_and_saveexec_b64 " LD_SW ", vcc\n\t"                       \
    "s_cbranch_execz .Lrf" N "_%=\n\t"                            \
    "v_and_b32_e32 " WR ", 0xffffff00, " LD_PROD "\n\t"           \
    LD_TAKE                                                       \
    ".Lrf" N "_%=:\n\t"                                           \
    "s_mov_b64 exec, " LD_SW "\n\t"
// one bin of the nested unary prefix (slots 1..3): a 1 = the lane stays, with its range in WR
#define LD_UNARY(EL, EH, OFS, N, SAVE, RD, WR)                              \
    LD_SPLIT_TO(EL, RD, WR)                                                 \
    "v_sub_co_u32_e32 " LD_LOW ", vcc, " LD_LOW ", " RD "\n\t"              \
    "ds_write_b16_d16_hi %[bank], " EL " offset:" OFS "\n\t"                \
    "s_andn2_b64 exec, exec, vcc\n\t"                                       \
    SAVE                                                                    \
    "s_cbranch_execz .Lx_done_%=\n\t"                                       \
    "ds_write_b16_d16_hi %[bank], " EH " offset:" OFS "\n\t"                \
    "v_add_u32_e32 " LD_EX ", 1, " LD_EX "\n\t"                             \
    LD_REFILL_R1(WR, N)
// entries of slots 1..7 from the bank words (addresses by mask / constant right shift)
#define LD_FETCH_REST                                         \
    "v_lshrrev_b32_e32 " LD_E1L ", 16, %[w0]\n\t"             \
    "v_and_b32_e32 " LD_E2L ", 0xffff, %[w1]\n\t"             \
    "v_lshrrev_b32_e32 " LD_E3L ", 16, %[w1]\n\t"             \
    "v_and_b32_e32 " LD_E4L ", 0xffff, %[w2]\n\t"             \
    "ds_read_b64 " LD_E1 ", " LD_E1L "\n\t"                   \
    "ds_read_b64 " LD_E2 ", " LD_E2L "\n\t"                   \
    "ds_read_b64 " LD_E3 ", " LD_E3L "\n\t"                   \
    "ds_read_b64 " LD_E4 ", " LD_E4L "\n\t"                   \
    "v_lshrrev_b32_e32 " LD_E5L ", 16, %[w2]\n\t"             \
    "v_and_b32_e32 " LD_E6L ", 0xffff, %[w3]\n\t"             \
    "v_lshrrev_b32_e32 " LD_E7L ", 16, %[w3]\n\t"             \
    "ds_read_b64 " LD_E5 ", " LD_E5L "\n\t"                   \
    "ds_read_b64 " LD_E6 ", " LD_E6L "\n\t"                   \
    "ds_read_b64 " LD_E7 ", " LD_E7L "\n\t"

// the sample's bytes at the head: the window's next three over the sentinel
#define LD_HEAD_COPY "v_perm_b32 " LD_CPY ", %[winl_in], %[winl_in], %[sel]\n\t"
#define LD_SEL 0x0001020Du  // bytes 0, 1, 2 of the window's low dword into bytes 3, 2, 1; the constant 0xFF into byte 0
// the bits that went: the lowest set bit of the copy  (a copy that is used up gives nonsense: that lane is replayed)
#define LD_TAIL_BITS "v_ffbl_b32_e32 " LD_DIFF ", " LD_CPY "\n\t"
// the run on slot 4, two bins per turn: the first reads its range from B and writes r1 to A (the lanes that leave on it join LD_SB),
// the second the other way round; both halves test for the end
#define LD_URUN                                                      \
    ".Lu_%=:\n\t"                                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    LD_SPLIT_TO(LD_E4L, LD_R1, "%[range]")                           \
    "v_sub_co_u32_e32 " LD_LOW ", vcc, " LD_LOW ", " LD_R1 "\n\t"    \
    "s_and_b64 " LD_SP ", exec, vcc\n\t"                             \
    "s_andn2_b64 exec, exec, vcc\n\t"                                \
    "s_or_b64 " LD_SB ", " LD_SB ", " LD_SP "\n\t"                   \
    "s_cbranch_execz .Lu_done_%=\n\t"                                \
    "v_lshrrev_b32_e32 " LD_OFF ", 16, " LD_E4H "\n\t"               \
    "ds_read_b64 " LD_E4 ", " LD_OFF "\n\t"                          \
    "v_add_u32_e32 " LD_EX ", 1, " LD_EX "\n\t"                      \
    LD_REFILL_R1("%[range]", "4")                                    \
    "s_waitcnt lgkmcnt(0)\n\t"                                       \
    LD_SPLIT_TO(LD_E4L, "%[range]", LD_R1)                           \
    "v_sub_co_u32_e32 " LD_LOW ", vcc, " LD_LOW ", %[range]\n\t"     \
    "s_andn2_b64 exec, exec, vcc\n\t"                                \
    "s_cbranch_execz .Lu_done_%=\n\t"                                \
    "v_lshrrev_b32_e32 " LD_OFF ", 16, " LD_E4H "\n\t"               \
    "ds_read_b64 " LD_E4 ", " LD_OFF "\n\t"                          \
    "v_add_u32_e32 " LD_EX ", 1, " LD_EX "\n\t"                      \
    LD_REFILL_R1(LD_R1, "4b")                                        \
    "s_branch .Lu_%=\n"
// LD_SB: nobody yet / the lanes that leave on slot 2 (they stayed behind slot 1 and not behind slot 2) / ... and their r0 goes over to A
#define LD_UNARY_INIT "s_mov_b64 " LD_SB ", 0\n\t"
#define LD_SAVE2 "s_mov_b64 " LD_SM ", exec\n\ts_andn2_b64 " LD_SB ", " LD_S1L ", exec\n\t"
#define LD_COLLECT                           \
    "s_mov_b64 exec, " LD_SB "\n\t"          \
    "v_mov_b32_e32 %[range], " LD_R1 "\n\t"

// The block's text.  LD_LOW / LD_CPY / LD_PAIR name the outgoing low, the sample's copy of the window bytes and the pair of the two.
#define LD_TEXT                                                                                                                    \
        "s_mov_b64 " LD_SX ", exec\n\t"                                                                                            \
        LD_HEAD_COPY                                                                                                               \
        "v_and_b32_e32 " LD_OFF ", 0xffff, %[w0]\n\t"                                                                              \
        "ds_read_b64 " LD_E0 ", " LD_OFF "\n\t"                                                                                    \
        "v_mov_b32_e32 %[value], 0\n\t"                                                                                            \
        "s_cmp_lg_u32 %[hot], 0\n\t"                                                                                               \
        "s_cbranch_scc0 .Lcold_%=\n\t"                                                                                             \
        LD_FETCH_REST                                                                                                              \
        "s_waitcnt lgkmcnt(7)\n\t"                                                                                                 \
        "s_branch .Lzero_%=\n"                                                                                                     \
        ".Lcold_%=:\n\t"                                                                                                           \
        "s_waitcnt lgkmcnt(0)\n"                                                                                                   \
        /* ---- slot 0: a 1 = the residual is zero (the lane is done), a 0 (borrow) = it goes on */                               \
        ".Lzero_%=:\n\t"                                                                                                           \
        /* (the outgoing low is the difference; the lanes with a borrow keep the incoming one -- the select stands where the */   \
        /* move of the difference stood, two instructions behind the v_sub_co that wrote VCC) */                                  \
        LD_SPLIT_IN(LD_E0L)                                                                                                        \
        "v_sub_co_u32_e32 " LD_LOW ", vcc, %[low_in], %[range]\n\t"                                                                \
        "ds_write_b16_d16_hi %[bank], " LD_E0L "\n\t"                                                                              \
        "s_and_b64 " LD_SA ", exec, vcc\n\t"                                                                                       \
        "v_cndmask_b32_e32 " LD_LOW ", " LD_LOW ", %[low_in], vcc\n\t"                                                             \
        "s_andn2_b64 exec, exec, vcc\n\t"                                                                                          \
        "s_cbranch_execz .Lz1_%=\n\t"                                                                                              \
        "v_mov_b32_e32 %[range], " LD_R1 "\n\t"                                                                                    \
        "ds_write_b16_d16_hi %[bank], " LD_E0H "\n"                                                                                \
        ".Lz1_%=:\n\t"                                                                                                             \
        "s_mov_b64 exec, " LD_SX "\n\t"                                                                                            \
        LD_REFILL("0")                                                                                                             \
        "s_and_b64 exec, " LD_SA ", " LD_SA "\n\t"                                                                                 \
        "s_cbranch_execz .Ldone_%=\n\t"                                                                                            \
        "s_cmp_lg_u32 %[hot], 0\n\t"                                                                                               \
        "s_cbranch_scc1 .Lhave_%=\n\t"                                                                                             \
        LD_FETCH_REST                                                                                                              \
        ".Lhave_%=:\n\t"                                                                                                           \
        "v_mov_b32_e32 " LD_EX ", 0\n\t"                                                                                           \
        "v_mov_b32_e32 " LD_W ", 1\n\t"                                                                                            \
        "s_waitcnt lgkmcnt(0)\n\t"                                                                                                 \
        /* ---- unary exponent: slots 1, 2, 3 once each, then a run on slot 4; the range alternates A -> B -> A -> B */            \
        /* (the lanes that stay behind slots 1 and 2 are the lanes of slot 5 and of the mantissa run: kept, not compared for */   \
        /* again; the lanes that LEAVE on slot 2 are the first whose r0 is in B) */                                               \
        "s_mov_b64 " LD_SM ", 0\n\t"                                                                                               \
        LD_UNARY_INIT                                                                                                              \
        LD_UNARY(LD_E1L, LD_E1H, "2", "1", "s_mov_b64 " LD_S1L ", exec\n\t", "%[range]", LD_R1)                                   \
        LD_UNARY(LD_E2L, LD_E2H, "256", "2", LD_SAVE2, LD_R1, "%[range]")                                                          \
        LD_UNARY(LD_E3L, LD_E3H, "258", "3", "", "%[range]", LD_R1)                                                                \
        "s_mov_b64 " LD_SU ", exec\n\t"                                                                                            \
        ".p2align 6\n"                                                                                                             \
        LD_URUN                                                                                                                    \
        ".Lu_done_%=:\n\t"                                                                                                         \
        "s_mov_b64 exec, " LD_SU "\n\t"                                                                                            \
        "ds_write_b16_d16_hi %[bank], " LD_E4L " offset:512\n" /* slot 4: the closing 0's successor */                            \
        ".Lx_done_%=:\n\t"                                                                                                         \
        LD_COLLECT                                                                                                                 \
        "s_mov_b64 exec, " LD_SA "\n\t"                                                                                            \
        "v_add_u32_e32 " LD_LOW ", " LD_LOW ", %[range]\n\t" /* every lane left by a borrow, with low - r0: put r0 back ... */    \
        LD_REFILL("5")                                       /* ... and refill behind the closing 0 */                            \
        /* ---- exponent > 31: "Invalid exponent" -- the lane stops here (rare; the caller replays it) */                         \
        "v_cmp_lt_u32_e32 vcc, 31, " LD_EX "\n\t"                                                                                  \
        "s_cbranch_vccz .Lexok_%=\n\t"                                                                                             \
        "s_and_saveexec_b64 " LD_SP ", vcc\n\t"                                                                                    \
        "v_mov_b32_e32 " LD_CPY ", 0\n\t" /* used-up bytes (not even the sentinel left) are what makes the caller replay */       \
        "s_andn2_b64 exec, " LD_SP ", exec\n\t"                                                                                    \
        "s_cbranch_execz .Ldone_%=\n"                                                                                              \
        ".Lexok_%=:\n\t"                                                                                                           \
        "s_mov_b64 " LD_S5 ", exec\n\t" /* (the lanes that finish the sample: value and sign below) */                            \
        /* ---- slot 5: the mantissa bit below the leading one (exponent > 0); w = 2 + inverted bit */                            \
        "s_and_b64 exec, exec, " LD_S1L "\n\t" /* exponent > 0 */                                                                 \
        "s_cbranch_execz .Lvalue_%=\n\t"                                                                                           \
        "s_mov_b64 " LD_SU ", exec\n\t"                                                                                            \
        LD_SPLIT(LD_E5L)                                                                                                           \
        "v_sub_co_u32_e32 " LD_DIFF ", vcc, " LD_LOW ", %[range]\n\t"                                                              \
        "ds_write_b16_d16_hi %[bank], " LD_E5L " offset:514\n\t"                                                                   \
        "s_andn2_b64 " LD_SP ", exec, vcc\n\t"                         /* the lanes that decoded a 1 */                           \
        "v_addc_co_u32_e32 " LD_W ", vcc, " LD_W ", " LD_W ", vcc\n\t" /* 1 + 1 + borrow */                                       \
        "v_mov_b32_e32 " LD_RUN ", 0\n\t"                                                                                          \
        "s_and_b64 exec, " LD_SP ", " LD_SP "\n\t"                                                                                 \
        "s_cbranch_execz .Lp5_%=\n\t"                                                                                              \
        "v_mov_b32_e32 " LD_LOW ", " LD_DIFF "\n\t"                                                                                \
        "v_mov_b32_e32 %[range], " LD_R1 "\n\t"                                                                                    \
        "ds_write_b16_d16_hi %[bank], " LD_E5H " offset:514\n"                                                                     \
        ".Lp5_%=:\n\t"                                                                                                             \
        "s_mov_b64 exec, " LD_SU "\n\t"                                                                                            \
        LD_REFILL("6")                                                                                                             \
        /* ---- the rest of the mantissa as a run on slot 6 (exponent > 1): bits gathered under a marker that leaves as a carry */ \
        "v_add_u32_e32 " LD_T ", -1, " LD_EX "\n\t" /* m = bins of the run */                                                     \
        "s_and_b64 exec, exec, " LD_SM "\n\t"       /* exponent > 1 */                                                            \
        "s_cbranch_execz .Lm_skip_%=\n\t"                                                                                          \
        "s_mov_b64 " LD_SP ", exec\n\t"                                                                                            \
        "v_add_u32_e32 " LD_NX ", -2, " LD_EX "\n\t"                                                                               \
        "v_lshrrev_b32_e32 " LD_RUN ", " LD_NX ", %[sentv]\n\t" /* marker at bit 32 - m */                                        \
        ".p2align 6\n"                                                                                                             \
        ".Lm_%=:\n\t"                                                                                                              \
        "s_waitcnt lgkmcnt(0)\n\t"                                                                                                 \
        LD_SPLIT(LD_E6L)                                                                                                           \
        "v_sub_co_u32_e32 " LD_DIFF ", vcc, " LD_LOW ", %[range]\n\t"                                                              \
        "s_nop 1\n\t" /* (VALU wrote VCC, VALU reads VCC: two wait states on gfx950) */                                           \
        "v_cndmask_b32_e32 %[range], " LD_R1 ", %[range], vcc\n\t"                                                                 \
        "v_cndmask_b32_e32 " LD_LOW ", " LD_DIFF ", " LD_LOW ", vcc\n\t"                                                           \
        "v_cndmask_b32_e32 " LD_NX ", " LD_E6H ", " LD_E6L ", vcc\n\t"                                                             \
        /* 2 run + borrow (inverted bits); carry out: this was the last bit */                                                    \
        "v_addc_co_u32_e32 " LD_RUN ", vcc, " LD_RUN ", " LD_RUN ", vcc\n\t"                                                       \
        "s_mov_b64 " LD_SD ", vcc\n\t"                                                                                             \
        "v_lshrrev_b32_e32 " LD_OFF ", 16, " LD_NX "\n\t"                                                                          \
        "ds_read_b64 " LD_E6 ", " LD_OFF "\n\t"                                                                                    \
        "v_cmp_gt_u32_e32 vcc, %[c100], %[range]\n\t"                                                                              \
        "s_and_saveexec_b64 " LD_SW ", vcc\n\t"                                                                                    \
        "s_cbranch_execz .Lmr_%=\n\t"                                                                                              \
        "v_lshlrev_b32_e32 %[range], 8, %[range]\n\t"                                                                              \
        LD_TAKE                                                                                                                    \
        ".Lmr_%=:\n\t"                                                                                                             \
        "s_andn2_b64 exec, " LD_SW ", " LD_SD "\n\t" /* everybody back, minus the lanes that are done */                          \
        "s_cbranch_execnz .Lm_%=\n\t"                                                                                              \
        "s_mov_b64 exec, " LD_SP "\n\t"                                                                                            \
        "ds_write_b16_d16_hi %[bank], " LD_NX " offset:768\n" /* slot 6: the successor the last bin chose */                      \
        ".Lm_skip_%=:\n\t"                                                                                                         \
        "s_mov_b64 exec, " LD_SU "\n\t"                                                                                            \
        "v_lshlrev_b32_e32 " LD_W ", " LD_T ", " LD_W "\n\t" /* what was gathered before the run moves up to make room for it */  \
        "v_or_b32_e32 " LD_W ", " LD_W ", " LD_RUN "\n"                                                                            \
        /* ---- the value: w with the bits below its leading one inverted back (w == 1 for exponent 0) */                         \
        ".Lvalue_%=:\n\t"                                                                                                          \
        "s_mov_b64 exec, " LD_S5 "\n\t"                                                                                            \
        "v_lshlrev_b32_e64 " LD_T ", " LD_EX ", 1\n\t"                                                                             \
        "v_add_u32_e32 " LD_T ", -1, " LD_T "\n\t"                                                                                 \
        "v_xor_b32_e32 %[value], " LD_W ", " LD_T "\n\t"                                                                           \
        /* ---- slot 7: the sign (a 1 = negative) */                                                                              \
        LD_SPLIT(LD_E7L)                                                                                                           \
        "v_sub_co_u32_e32 " LD_DIFF ", vcc, " LD_LOW ", %[range]\n\t"                                                              \
        "ds_write_b16_d16_hi %[bank], " LD_E7L " offset:770\n\t"                                                                   \
        "s_andn2_b64 exec, exec, vcc\n\t"                                                                                          \
        "s_cbranch_execz .Lp7_%=\n\t"                                                                                              \
        "v_mov_b32_e32 " LD_LOW ", " LD_DIFF "\n\t"                                                                                \
        "v_mov_b32_e32 %[range], " LD_R1 "\n\t"                                                                                    \
        "ds_write_b16_d16_hi %[bank], " LD_E7H " offset:770\n\t"                                                                   \
        "v_sub_u32_e32 %[value], 0, %[value]\n"                                                                                    \
        ".Lp7_%=:\n\t"                                                                                                             \
        "s_mov_b64 exec, " LD_S5 "\n\t"                                                                                            \
        LD_REFILL("7")                                                                                                             \
        ".Ldone_%=:\n\t"                                                                                                           \
        "s_mov_b64 exec, " LD_SX "\n\t"                                                                                            \
        LD_TAIL_BITS                                                                                                               \
        "v_lshrrev_b64 %[win], " LD_DIFF ", %[win_in]\n\t" /* the 64-bit window moves once, by the bytes that went */             \
        "s_bcnt1_i32_b64 " LD_S1 ", " LD_SA "\n\t"                                                                                 \
        "s_bcnt1_i32_b64 " LD_S2 ", " LD_SX "\n\t"                                                                                 \
        "s_lshl_b32 " LD_S1 ", " LD_S1 ", 1\n\t"                                                                                   \
        "s_cmp_ge_u32 " LD_S1 ", " LD_S2 "\n\t"                                                                                    \
        "s_cselect_b32 %[hot], 1, 0\n\t"                                                                                           \
        "s_mov_b64 exec, " LD_SX "\n\t"
#define LD_INPUTS                                                                                                                   \
    [low_in] "v"(low_in), [range_in] "v"(range_in), [win_in] "v"(win_in), [winl_in] "v"(uint32_t(win_in)), [w0] "v"(w0), [w1] "v"(w1), \
        [w2] "v"(w2), [w3] "v"(w3), [bank] "v"(bank), [c100] "s"(0x100u), [sel] "s"(LD_SEL), [sentv] "v"(0x80000000u)
#define LD_CLOBBERS                                                                                                                 \
    "vcc", "scc", "memory", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v48", \
        "v49", "v50", "v51", "v52", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", \
        "s70", "s71"

// in: exec = the lanes of the wavefront's slices; low_in / range_in / win_in as in RangeDec (left untouched; range / win: the same
// behind the sample); w0..w3 = the context's wide row bank (read by the caller, who also needs it to roll back), bank = its LDS
// address; hot = wave-uniform "most lanes had a non-zero residual last time" (in: entries of slots 1..7 are requested up front;
// out: the new flag).  out: value = the decoded residual's magnitude with the sign bin applied (0 for a zero residual);
// low_copy = low behind the sample (high dword) over what is left of the sample's private copy of the window's next three bytes
// (low dword; see the header): 0 there = the sample wanted more than the three, or its exponent exceeded 31 ("Invalid exponent",
// llcomp.hpp:230-235: the lane stops behind the exponent) -- the caller replays that lane on the checked path.
// SET: which of the block's two fixed register pairs low_copy leaves in.
#define LD_BLOCK(PAIR)                                                                                                        \
    asm volatile(LD_TEXT : [lc] "=&{" PAIR "}"(low_copy), [range] "=&v"(range), [win] "=&v"(win), [hot] "+s"(hot), [value] "=&v"(value) \
                 : LD_INPUTS                                                                                                  \
                 : LD_CLOBBERS)
// the replay's start: the untouched inputs IN the registers of the block's outputs (see dec_sample)
#define LD_REPLAY_COPY(PAIR)                                                                  \
    asm("v_mov_b32_e32 " LD_LOW ", %3\n\tv_mov_b32_e32 %1, %4\n\tv_mov_b64_e32 %2, %5"        \
        : "+{" PAIR "}"(low_copy), "+v"(range), "+v"(win)                                     \
        : "v"(low_in), "v"(range_in), "v"(win_in))
template <int SET>
__device__ __forceinline__ void dec_rows_sample_asm(uint32_t low_in, uint32_t range_in, unsigned long long win_in,
                                                    unsigned long long& low_copy, uint32_t& range, unsigned long long& win, uint32_t w0,
                                                    uint32_t w1, uint32_t w2, uint32_t w3, uint32_t bank, uint32_t& hot, uint32_t& value) {
    if constexpr (SET == 0) {
#define LD_PAIR "v[0:1]"
#define LD_CPY "v0"
#define LD_LOW "v1"
        LD_BLOCK("v[0:1]");
    } else {
#undef LD_PAIR
#undef LD_CPY
#undef LD_LOW
#define LD_PAIR "v[2:3]"
#define LD_CPY "v2"
#define LD_LOW "v3"
        LD_BLOCK("v[2:3]");
    }
}
template <int SET>
__device__ __forceinline__ void dec_rows_replay_inputs(uint32_t low_in, uint32_t range_in, unsigned long long win_in,
                                                       unsigned long long& low_copy, uint32_t& range, unsigned long long& win) {
    if constexpr (SET == 0) {
#undef LD_LOW
#define LD_LOW "v1"
        LD_REPLAY_COPY("v[0:1]");
    } else {
#undef LD_LOW
#define LD_LOW "v3"
        LD_REPLAY_COPY("v[2:3]");
    }
}

}  // namespace llcomp_mi
