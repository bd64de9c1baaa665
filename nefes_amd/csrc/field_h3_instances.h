// The compiled instances of the fp16 two-part field kernels (field_fwd_h3.hip, field_bwd_h3.hip): ONE table per direction.
// Both sources are built once per `part` (Makefile: -DNEFES_TU_PART=<part> -> field_{fwd,bwd}_h3.p<part>.o); a part's object
// instantiates the rows that name it and defines their launch function, part 0 also holds the entry points.  Launchers, the
// selectors' lookup and nefes_field_h3_instance are generated from the rows; nothing else names an instance.
// A new instance = one row here, plus a Makefile entry (H3_W256 / H3_W128) if it needs a new part.  Part membership decides the
// flags an instance is compiled with, so a row never moves to another part:
//   - the even parts from 2 on are built for Wd = 128 (NEFES_TU_W128: 16 KiB slabs, -amdgpu-mfma-vgpr-form and, backward, the
//     block-per-pair form for every segment); every other part for Wd = 256 (32 KiB slabs);
//   - of the backward's Wd = 256 parts, those without TRAIN rows run the gap-by-gap schedule (NEFES_TU_BWD_WIDE).
// Both sources static-assert these rules against their rows.
#pragma once

#ifndef NEFES_TU_PART
#define NEFES_TU_PART 0
#endif
#if NEFES_TU_PART >= 2 && NEFES_TU_PART % 2 == 0
#define NEFES_TU_W128
#elif NEFES_TU_PART == 0 || NEFES_TU_PART == 1 || NEFES_TU_PART == 5 || NEFES_TU_PART == 9 || \
    NEFES_TU_PART == 11 || NEFES_TU_PART == 13
#define NEFES_TU_BWD_WIDE
#endif

// kernel-internal values of the template parameters, next to the public NEFES_FIELD_* / NEFES_XYZ_* ones
#define NEFES_XYZ_HASHGRID_FUSED 2   /* ENC: a NEFES_XYZ_EXTERNAL32 network whose 32 hash-grid features the kernel evaluates itself */
#define NEFES_FIELD_FULL_FOLD 3      /* forward MODE: the full pass on a folded pack (NefesNetDesc.fold_final) */
#define NEFES_H3B_FOLD 16            /* backward: the same, carried in the head-class parameter (KR16 | NEFES_H3B_FOLD) */

// A row's key is the tuple of template arguments itself.
struct NefesH3FwdKey { int mode, enc, w, ntr, train, fh; };
struct NefesH3BwdKey { int w, kr16, enc, has_t, train, fh; };
inline bool operator==(const NefesH3FwdKey& a, const NefesH3FwdKey& b) {
    return a.mode == b.mode && a.enc == b.enc && a.w == b.w && a.ntr == b.ntr && a.train == b.train && a.fh == b.fh;
}
inline bool operator==(const NefesH3BwdKey& a, const NefesH3BwdKey& b) {
    return a.w == b.w && a.kr16 == b.kr16 && a.enc == b.enc && a.has_t == b.has_t && a.train == b.train && a.fh == b.fh;
}

// X(part, MODE, ENC, W, NTR, TRAIN, FH): MODE / ENC without their NEFES_FIELD_ / NEFES_XYZ_ prefix; NTR = tiles of the rgb+feature
// head = the head class of layout.h (1: 3 + C <= 32; 5: 3 + C <= 144).  The sigma-only pass has no rgb head: one row per width and
// encoding serves both head classes.
#define NEFES_H3_FWD_INSTANCES(X)                                                                                                  \
    X(0, SIGMA, FREQ10, 256, 1, 0, 0)                                                                                              \
    X(0, FULL, FREQ10, 256, 1, 0, 0)                                                                                               \
    X(1, SIGMA, EXTERNAL32, 256, 1, 0, 0)                                                                                          \
    X(1, FULL, EXTERNAL32, 256, 1, 0, 0)                                                                                           \
    /* the static head alone at inference: what a frozen coarse network runs when test_time is False (rendering.py:116-125) and a  \
       fine network with NeRFW off (nerfh_nff.py:217-231 with output_transient False) -- the TRAIN rows' kernel without the        \
       activation stores */                                                                                                        \
    X(1, STATIC, FREQ10, 256, 1, 0, 0)                                                                                             \
    /* the hash grid gathered in the prologue */                                                                                   \
    X(1, SIGMA, HASHGRID_FUSED, 256, 1, 0, 0)                                                                                      \
    X(1, FULL, HASHGRID_FUSED, 256, 1, 0, 0)                                                                                       \
    /* The Wd = 128 instances hold 2 x 4 accumulator tiles = 128 registers: with ~120 more for everything else the whole kernel    \
       fits the 256 architectural VGPRs, and the Wd = 128 objects are built with -mllvm -amdgpu-mfma-vgpr-form (Makefile) so that  \
       the MFMAs accumulate there.  Left to its heuristics hipcc parks the tiles in AGPRs and pays a v_accvgpr_read / _write for   \
       every value the vector ALU touches (1.7 of the kernel's 6.3 VALU per MFMA: it is VALU-bound at this width): forward         \
       0.85 -> 0.78 ms, backward 0.77 -> 0.73 ms on the 80x60 refinement frame. */                                                 \
    X(2, SIGMA, FREQ10, 128, 5, 0, 0)                                                                                              \
    X(2, FULL, FREQ10, 128, 5, 0, 0)                                                                                               \
    X(2, STATIC, FREQ10, 128, 5, 0, 0)                                                                                             \
    X(3, STATIC, FREQ10, 256, 1, 1, 0)                                                                                             \
    X(3, FULL, FREQ10, 256, 1, 1, 0)                                                                                               \
    /* an external 32-feature encoding (a trainable hash grid): its features go to the E block in natural order (compact slot      \
       (s, h) = feature 2s + h = row 2s + h) */                                                                                    \
    X(3, STATIC, EXTERNAL32, 256, 1, 1, 0)                                                                                         \
    X(3, FULL, EXTERNAL32, 256, 1, 1, 0)                                                                                           \
    X(4, STATIC, FREQ10, 128, 5, 1, 0)                                                                                             \
    X(4, FULL, FREQ10, 128, 5, 1, 0)                                                                                               \
    /* the reference's FEATURE_DIM = 128 at netwidth 256 */                                                                        \
    X(5, FULL, FREQ10, 256, 5, 0, 0)                                                                                               \
    X(5, STATIC, FREQ10, 256, 5, 0, 0)                                                                                             \
    X(6, FULL, FREQ10, 128, 1, 0, 0)                                                                                               \
    X(6, STATIC, FREQ10, 128, 1, 0, 0)                                                                                             \
    X(6, FULL, FREQ10, 128, 1, 0, 1) /* factored head (the kernel's FH parameter) */                                               \
    X(7, STATIC, FREQ10, 256, 5, 1, 0)                                                                                             \
    X(7, FULL, FREQ10, 256, 5, 1, 0)                                                                                               \
    X(8, STATIC, FREQ10, 128, 1, 1, 0)                                                                                             \
    X(8, FULL, FREQ10, 128, 1, 1, 0)                                                                                               \
    X(9, FULL_FOLD, FREQ10, 256, 1, 0, 0)                                                                                          \
    X(11, FULL_FOLD, FREQ10, 256, 5, 0, 0)                                                                                         \
    /* The reference's FEATURE_DIM = 128 on a hash grid: the full pass with the five-tile rgb+feature head on a SUPPLIED encoding. \
       No fused-gather instance of this class: its forward <FULL, HASHGRID_FUSED, 256, 5> builds clean (256 + 256 registers, no    \
       scratch), its backward does not keep the house rules (the backward table below), and a forward alone would leave the pair's \
       masks without a consumer -- DESIGN.md 4.8.  Experiments: make EXTRA_H3=-DNEFES_H3_HG_CLASS1 builds the pair, and the        \
       class-1 full pass of the _hashgrid entry points then finds its row (re-check the registers with tools/kernel_resources.py   \
       and the moves with tools/hazard_lint.py after a compiler update). */                                                        \
    X(13, FULL, EXTERNAL32, 256, 5, 0, 0)                                                                                          \
    NEFES_H3_FWD_HG_CLASS1(X)                                                                                                      \
    X(15, STATIC, EXTERNAL32, 256, 5, 1, 0)                                                                                        \
    X(15, FULL, EXTERNAL32, 256, 5, 1, 0)

// X(part, W, KR16, ENC, HAS_T, TRAIN, FH): KR16 = k-steps of 16 upstream channels of static_rgb^T = the head class (2: 3 + C <= 32;
// 9: 3 + C <= 144), | NEFES_H3B_FOLD on a folded pack; HAS_T = 0: the static head only (the backward of a NEFES_FIELD_STATIC forward).
#define NEFES_H3_BWD_INSTANCES(X)                                                                                                  \
    X(0, 256, 2, FREQ10, 1, 0, 0)                                                                                                  \
    X(1, 256, 2, EXTERNAL32, 1, 0, 0)                                                                                              \
    X(1, 256, 2, FREQ10, 0, 0, 0)                                                                                                  \
    /* The hash grid's backward in the epilogue, on the gap-by-gap schedule like its neighbours.  Its first form parked the skip   \
       connection's share of d encoding in LDS across layers 4..1 and hipcc then split an accumulator tile's live range inside an  \
       asm-scheduled run (a v_accvgpr_mov behind an MFMA that has not written the tile yet: tests/test_pack_stream.py caught it,   \
       no numerical test did); with the share in sixteen registers, as the external-encoding instance keeps it, the tiles stay     \
       put. */                                                                                                                     \
    X(1, 256, 2, HASHGRID_FUSED, 1, 0, 0)                                                                                          \
    X(2, 128, 9, FREQ10, 1, 0, 0)                                                                                                  \
    X(2, 128, 9, FREQ10, 0, 0, 0)                                                                                                  \
    X(3, 256, 2, FREQ10, 0, 1, 0)                                                                                                  \
    X(3, 256, 2, FREQ10, 1, 1, 0)                                                                                                  \
    X(3, 256, 2, EXTERNAL32, 0, 1, 0) /* trainable hash grid */                                                                    \
    X(3, 256, 2, EXTERNAL32, 1, 1, 0)                                                                                              \
    X(4, 128, 9, FREQ10, 0, 1, 0)                                                                                                  \
    X(4, 128, 9, FREQ10, 1, 1, 0)                                                                                                  \
    X(5, 256, 9, FREQ10, 1, 0, 0)                                                                                                  \
    X(5, 256, 9, FREQ10, 0, 0, 0)                                                                                                  \
    X(6, 128, 2, FREQ10, 1, 0, 0)                                                                                                  \
    X(6, 128, 2, FREQ10, 0, 0, 0)                                                                                                  \
    X(6, 128, 2, FREQ10, 1, 0, 1) /* factored head */                                                                              \
    X(7, 256, 9, FREQ10, 0, 1, 0)                                                                                                  \
    X(7, 256, 9, FREQ10, 1, 1, 0)                                                                                                  \
    X(8, 128, 2, FREQ10, 0, 1, 0)                                                                                                  \
    X(8, 128, 2, FREQ10, 1, 1, 0)                                                                                                  \
    X(9, 256, 2 | NEFES_H3B_FOLD, FREQ10, 1, 0, 0)                                                                                 \
    X(11, 256, 9 | NEFES_H3B_FOLD, FREQ10, 1, 0, 0)                                                                                \
    /* Head class 1 on a SUPPLIED encoding.  The instance with the hash grid in its epilogue, <256, 9, HASHGRID_FUSED>, is not     \
       built: on the gap-by-gap schedule hipcc relocates accumulator tiles inside the asm-scheduled runs (v_accvgpr_mov one to six \
       wait states behind the asm MFMA that writes the tile: tools/hazard_lint.py rule B1 -- 512 registers, no scratch), the       \
       failure the class-0 instance avoids by leaving the schedule, and the seventy-two upstream values of this class leave it     \
       less room, not more.  Such networks take nefes_hashgrid_fwd / _bwd_x around the EXTERNAL32 instance                         \
       (ops.hashgrid_fused_ok).  make EXTRA_H3=-DNEFES_H3_HG_CLASS1 builds it (experiments: the linter and          \
       tests/test_pack_stream.py are red on that library). */                                                                      \
    X(13, 256, 9, EXTERNAL32, 1, 0, 0)                                                                                             \
    NEFES_H3_BWD_HG_CLASS1(X)                                                                                                      \
    X(15, 256, 9, EXTERNAL32, 0, 1, 0)                                                                                             \
    X(15, 256, 9, EXTERNAL32, 1, 1, 0)

#ifdef NEFES_H3_HG_CLASS1
#define NEFES_H3_FWD_HG_CLASS1(X) X(13, FULL, HASHGRID_FUSED, 256, 5, 0, 0)
#define NEFES_H3_BWD_HG_CLASS1(X) X(13, 256, 9, HASHGRID_FUSED, 1, 0, 0)
#else
#define NEFES_H3_FWD_HG_CLASS1(X)
#define NEFES_H3_BWD_HG_CLASS1(X)
#endif

// the launch function of a part's rows, defined by that part's object
#define NEFES_H3_PASTE_(a, b) a##b
#define NEFES_H3_PASTE(a, b) NEFES_H3_PASTE_(a, b)
#define NEFES_H3_FWD_PART_FN(part) NEFES_H3_PASTE(nefes_fwd_h3_launch_part, part)
#define NEFES_H3_BWD_PART_FN(part) NEFES_H3_PASTE(nefes_bwd_h3_launch_part, part)

#define NEFES_H3_FWD_KEY(MODE, ENC, W, NTR, TRAIN, FH) NefesH3FwdKey{NEFES_FIELD_##MODE, NEFES_XYZ_##ENC, W, NTR, TRAIN, FH}
#define NEFES_H3_BWD_KEY(W, KR16, ENC, HAS_T, TRAIN, FH) NefesH3BwdKey{W, KR16, NEFES_XYZ_##ENC, HAS_T, TRAIN, FH}
