// The two-phase k-loop of the hand-specialised kernels and the tile scaffold around it: the persistent loop of kernels_gemm_x3p.hip
// (D3D_PHASE, WPF form) for whole tiles -- eight waves (2 x 4) of 16 QF_TM rows x 16 QF_NJ columns (256 x 192 / 256 x 256 / 192 x 256
// stages), W fragments a phase ahead, counted vmcnt waits.  Users: the plain GEMMs kernels_proj_x3.hip, kernels_fc1_x3.hip,
// kernels_gemm_bf16q.hip and the fused qkv + attention kernels kernels_qkv_sattn.hip, kernels_qkv_tattn.hip, kernels_qkv_attn_bf16.hip.
// Macros only (expanded in the kernels, which include kloop_common.h inside their namespace): the kernels depend on WHERE the compiler
// re-derives per-lane offsets (the tid_o and lofs_ pins), which inline functions would not keep.
//
// A kernel binds its shape once with QF_SHAPE and then reads, per tile of its persistent walk:
//   QF_TILE_LANES; QF_TILE_NEXT(mtn, ntn); QF_TILE_PLAN(...); QF_TILE_ACC; int issued_prev = ...;
//   QF_KLOOP_HEAD(QF_PIECE)   k-tiles 0 .. nk - 2 (declares kt)
//   [row statistics reduced here, in the shadow of the SIMD partner's MFMAs]
//   QF_KLOOP_TAIL(QF_PIECE)   the last k-tile
// with QF_STAGE_FIRST in front of the walk.  A kernel with its own row map (gathered or strided A rows) writes its own plan and piece
// macro and passes that to QF_KLOOP_HEAD / QF_KLOOP_TAIL; the names every piece macro and the loop need in scope are those QF_TILE_PLAN
// and QF_TILE_ACC declare, plus lds, nk, has_next and issued_prev.
#pragma once

// QF_MMA(ACC, BH, BL, AH, AL) (optional): the products of one (m-tile, n-tile) pair for one staged 128-byte line of each operand row.
// Default: F16X3 -- the line holds the 32 hi and the 32 lo halves of a 32-deep k-tile: a_lo b_hi + a_hi b_lo + a_hi b_hi, smallest terms
// first.  kernels_gemm_bf16q.hip defines the bf16 form (the line holds 64 bf16 k values: one MFMA per 16-byte fragment pair).
#ifndef QF_MMA
#define QF_MMA(ACC, BH, BL, AH, AL)                                                                                      \
  do {                                                                                                                   \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BH, AL, ACC, 0, 0, 0);                                                  \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BL, AH, ACC, 0, 0, 0);                                                  \
    ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BH, AH, ACC, 0, 0, 0);                                                  \
  } while (0)
#endif

// ---- the tile scaffold ------------------------------------------------------------------------------------------------------------
// The shape of a kernel, bound once at namespace scope: a wave owns 16 TM rows x 16 NJ columns of the BM x BN tile; a k-tile is staged
// as AIT + BIT 1-KiB DMA pieces per wave.  A stage is BM rows of A, then (from byte QF_AREG on) BN rows of W, 128 bytes each.
#define QF_SHAPE(TM, NJ, BM, BN, AIT, BIT)                                                                               \
  constexpr int QF_TM = (TM), QF_NJ = (NJ), QF_BM = (BM), QF_BN = (BN), QF_AIT = (AIT), QF_BIT = (BIT);                  \
  constexpr int QF_AREG = QF_BM * 128, QF_STAGE = (QF_BM + QF_BN) * 128

// First k-tile of a walk's first tile, whose A / W rows start at ROWA / ROWB (in scope: K2, 16-bit words per operand row): the pieces
// of KL_DMA_PLAN (kloop_common.h), with the lane offset formed in front of the bases -- the order the instruction schedule was tuned with
#define QF_STAGE_FIRST(AP, WP, ROWA, ROWB)                                                                               \
  {                                                                                                                      \
    const int lane = threadIdx.x & 63;                                                                                   \
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);                                              \
    const int lr = lane >> 3, csrc = (lane & 7) ^ (((wave & 1) << 2) | (lr >> 1));                                       \
    const unsigned lofs = (unsigned)(lr * (int)K2 + csrc * 8) * 2u;                                                      \
    const char* ubA = reinterpret_cast<const char*>(AP) + (size_t)((ROWA) + wave * 8) * K2 * 2;                          \
    const char* ubB = reinterpret_cast<const char*>(WP) + (size_t)((ROWB) + wave * 8) * K2 * 2;                          \
    const size_t it_stride = (size_t)64 * K2 * 2;                                                                        \
    _Pragma("unroll") for (int it = 0; it < QF_AIT; ++it)                                                                \
      KL_GLDS(sgpr_ptr(ubA + it * it_stride) + lofs, wave * 1024 + lane * 16 + it * 8192);                               \
    _Pragma("unroll") for (int it = 0; it < QF_BIT; ++it)                                                                \
      KL_GLDS(sgpr_ptr(ubB + it * it_stride) + lofs, QF_AREG + wave * 1024 + lane * 16 + it * 8192);                     \
  }

// Top of a tile (in scope: int tid_o = threadIdx.x, declared in front of the walk): per-lane offsets are re-derived in every tile
// instead of being hoisted (and spilled)
#define QF_TILE_LANES                                                                                                    \
    asm volatile("" : "+v"(tid_o));                                                                                      \
    const int tid = tid_o;                                                                                               \
    const int lane = tid & 63;                                                                                           \
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);                                                           \
    const int wm = wave >> 2, wn = wave & 3;                                                                             \
    const int r16 = lane & 15, q = lane >> 4
// the walk's next tile (in scope: item, nitems, G, b, tile_of): its first k-tile is staged by the last phases of this tile's k-loop
#define QF_TILE_NEXT(MTN, NTN)                                                                                           \
    const bool has_next = item + 1 < nitems;                                                                             \
    int MTN = 0, NTN = 0;                                                                                                \
    if (has_next) tile_of((item + 1) * G + b, MTN, NTN)
// the DMA plan (kloop_common.h KL_DMA_PLAN) of the tile whose A / W rows start at ROWA / ROWB, and the bases of the next tile's
#define QF_TILE_PLAN(AP, WP, ROWA, ROWB, ROWA_NEXT, ROWB_NEXT)                                                           \
    KL_DMA_PLAN(AP, WP, K2, ROWA, ROWB, 8, QF_AREG);                                                                     \
    const char* ubAn = reinterpret_cast<const char*>(AP) + (size_t)((ROWA_NEXT) + wave * 8) * K2 * 2;                    \
    const char* ubBn = reinterpret_cast<const char*>(WP) + (size_t)((ROWB_NEXT) + wave * 8) * K2 * 2
// piece IT (A: 0 .. QF_AIT - 1, W: QF_AIT ..) of k-tile KTT of this tile, or (KTT == nk) of k-tile 0 of the next one
#define QF_PIECE(KTT, IT)                                                                                                \
    do {                                                                                                                 \
      const bool nxt_ = (KTT) >= nk;                                                                                     \
      const int st_ = ((KTT) & 1) * QF_STAGE;                                                                            \
      if ((IT) < QF_AIT) {                                                                                               \
        const char* b_ = nxt_ ? ubAn + (IT) * it_stride : ubA + ((size_t)(KTT) * 128 + (IT) * it_stride);                \
        KL_GLDS(sgpr_ptr(b_) + lofs_, st_ + dstA + (IT) * 8192);                                                         \
      } else {                                                                                                           \
        const char* b_ = nxt_ ? ubBn + ((IT) - QF_AIT) * it_stride : ubB + ((size_t)(KTT) * 128 + ((IT) - QF_AIT) * it_stride); \
        KL_GLDS(sgpr_ptr(b_) + lofs_, st_ + dstB + ((IT) - QF_AIT) * 8192);                                              \
      }                                                                                                                  \
    } while (0)
// zeroed accumulators, this lane's fragment offsets into a stage, the fragment registers.  (A kernel that needs its wave's first tile
// row again writes it as here, `wm * 16 * QF_TM`: one value for the compiler, which otherwise folds the two forms differently.)
#define QF_TILE_ACC                                                                                                     \
    f32x4 acc[QF_TM][QF_NJ];                                                                                             \
    _Pragma("unroll") for (int i = 0; i < QF_TM; ++i)                                                                    \
      _Pragma("unroll") for (int j = 0; j < QF_NJ; ++j)                                                                  \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.0f;                                               \
    const int foff = (q ^ (r16 >> 1)) << 4;                                                                              \
    const int aoff = (wm * 16 * QF_TM + r16) * 128 + foff, boff = QF_AREG + (wn * (16 * QF_NJ) + r16) * 128 + foff;      \
    h8 bh[QF_NJ], bl[QF_NJ], ah[2], al[2]

// ---- the plain GEMM kernels (proj, fc1, the bf16 token GEMM): whole tiles, contiguous rows ------------------------------------------
// The walk over MTILES x NTILES tiles of pair-layout operands AP / WP with K_ pairs per row, in the order of k_linear_x3q_persist:
// declares G, b, nitems, tile_of, K, K2, nk, the first tile (mt, nt) -- its first k-tile staged -- and tid_o.  Leaves when the
// workgroup has no tile.
#define QF_GEMM_WALK(AP, WP, MTILES, NTILES, K_)                                                                         \
  const int G = (int)gridDim.x, b = (int)blockIdx.x;                                                                     \
  const int ntiles = (NTILES), tiles = (MTILES) * ntiles;                                                                \
  if (b >= tiles) return;                                                                                                \
  const int nitems = (tiles - b + G - 1) / G;                                                                            \
  KL_XCD_TILE_ORDER(MTILES, ntiles);                                                                                     \
  const int K = (K_);                                                                                                    \
  const size_t K2 = 2 * (size_t)K;              /* 16-bit words per operand row */                                       \
  const int nk = K / 32;                                                                                                 \
  int mt = 0, nt = 0;                                                                                                    \
  tile_of(b, mt, nt);                                                                                                    \
  QF_STAGE_FIRST(AP, WP, mt * QF_BM, nt * QF_BN)                                                                         \
  int tid_o = (int)threadIdx.x
// Top of tile (mt, nt): lane indices, the next tile (mtn, ntn), the tile's first row / column m0 / n0
#define QF_GEMM_TILE_TOP                                                                                                 \
    QF_TILE_LANES;                                                                                                       \
    QF_TILE_NEXT(mtn, ntn);                                                                                              \
    const int m0 = mt * QF_BM, n0 = nt * QF_BN
// its DMA plan, accumulators and fragment offsets: all the k-loop needs but issued_prev
#define QF_GEMM_TILE_PLAN(AP, WP)                                                                                        \
    QF_TILE_PLAN(AP, WP, m0, n0, mtn * QF_BM, ntn * QF_BN);                                                              \
    QF_TILE_ACC

    // one phase (kernels_gemm_x3p.hip D3D_PHASE, WPF form): H = 0: m-tiles 0-3 of k-tile KT, issues A(KT+1) (and all of W(1), ahead of
    // A(1), in a tile's first phase); H = 1: m-tiles 4-7, issues W(KT+2); the W fragments of KT+1 replace those of KT behind the
    // last group's MFMA triples (W_AHEAD), the odd phase's first A pair is requested by the last group of the even phase.  PIECE(KTT, IT)
    // issues DMA piece IT of k-tile KTT: QF_PIECE, or the kernel's own
#define QF_PHASE(PIECE, KT, H, DO_A, W_FULL1, DO_W, W_AHEAD)                                                             \
    do {                                                                                                                 \
      wait_vm(issued_prev);                                                                                              \
      __builtin_amdgcn_s_barrier();                                                                                      \
      __builtin_amdgcn_s_setprio(3);                                                                                     \
      asm volatile("" : "+v"(lofs_) : : "memory");                                                                       \
      const unsigned char* sb = lds + ((KT) & 1) * QF_STAGE;                                                             \
      constexpr int G0 = (H) * (QF_TM / 2), G1 = G0 + QF_TM / 2;                                                         \
      constexpr int SPG_ = (QF_AIT + QF_BIT + QF_TM / 2 - 1) / (QF_TM / 2);   /* piece slots per group, even phase (2 at QF_TM 8) */ \
      constexpr int WPG_ = (QF_BIT + QF_TM / 2 - 1) / (QF_TM / 2);             /* W pieces per group, odd phase (1 at QF_TM 8) */    \
      if ((H) == 0) {                                                                                                    \
        ah[0] = *reinterpret_cast<const h8*>(sb + aoff);                                                                 \
        al[0] = *reinterpret_cast<const h8*>(sb + (aoff ^ 64));                                                          \
        if (W_FULL1) {                                                                                                   \
          _Pragma("unroll") for (int j = 0; j < QF_NJ; ++j) {                                                            \
            bh[j] = *reinterpret_cast<const h8*>(sb + boff + j * 2048);                                                  \
            bl[j] = *reinterpret_cast<const h8*>(sb + ((boff + j * 2048) ^ 64));                                         \
          }                                                                                                              \
        }                                                                                                                \
      }                                                                                                                  \
      _Pragma("unroll") for (int g = G0; g < G1; ++g) {                                                                  \
        if (g + 1 < (((H) == 0) ? QF_TM : G1)) {                                                                         \
          ah[(g + 1) & 1] = *reinterpret_cast<const h8*>(sb + aoff + (g + 1) * 2048);                                    \
          al[(g + 1) & 1] = *reinterpret_cast<const h8*>(sb + ((aoff + (g + 1) * 2048) ^ 64));                           \
        }                                                                                                                \
        if ((H) == 0 && SPG_ == 2) {                                                                                     \
          _Pragma("unroll") for (int pp = 0; pp < 2; ++pp) {                                                             \
            const int sl = (g - G0) * 2 + pp;                                                                            \
            if (W_FULL1) {                                                                                               \
              if (sl < QF_BIT) PIECE((KT) + 1, QF_AIT + sl);                                                             \
              else if (sl < QF_AIT + QF_BIT) { if (DO_A) PIECE((KT) + 1, sl - QF_BIT); }                                 \
            } else if (sl < QF_AIT) { if (DO_A) PIECE((KT) + 1, sl); }                                                   \
          }                                                                                                              \
        } else if ((H) == 0) {       /* (three m-tile groups per phase: more slots per group) */                          \
          _Pragma("unroll") for (int pp = 0; pp < SPG_; ++pp) {                                                          \
            const int sl = (g - G0) * SPG_ + pp;                                                                         \
            if (W_FULL1) {                                                                                               \
              if (sl < QF_BIT) PIECE((KT) + 1, QF_AIT + sl);                                                             \
              else if (sl < QF_AIT + QF_BIT) { if (DO_A) PIECE((KT) + 1, sl - QF_BIT); }                                 \
            } else if (sl < QF_AIT) { if (DO_A) PIECE((KT) + 1, sl); }                                                   \
          }                                                                                                              \
        } else if (WPG_ == 1) {                                                                                          \
          if (g - G0 < QF_BIT) {                                                                                         \
            if (DO_W) PIECE((KT) + 2, QF_AIT + (g - G0));                                                                \
          }                                                                                                              \
        } else {                                                                                                         \
          _Pragma("unroll") for (int pp = 0; pp < WPG_; ++pp) {                                                          \
            const int wp = (g - G0) * WPG_ + pp;                                                                         \
            if (wp < QF_BIT) { if (DO_W) PIECE((KT) + 2, QF_AIT + wp); }                                                 \
          }                                                                                                              \
        }                                                                                                                \
        const bool w_ahead_ = (H) == 1 && g == G1 - 1 && (W_AHEAD);                                                      \
        _Pragma("unroll") for (int j = 0; j < QF_NJ; ++j) {                                                              \
          QF_MMA(acc[g][j], bh[j], bl[j], ah[g & 1], al[g & 1]);                                                         \
          if (w_ahead_) {                                                                                                \
            const unsigned char* sbn = lds + (((KT) + 1) & 1) * QF_STAGE;                                                \
            bh[j] = *reinterpret_cast<const h8*>(sbn + boff + j * 2048);                                                 \
            bl[j] = *reinterpret_cast<const h8*>(sbn + ((boff + j * 2048) ^ 64));                                        \
          }                                                                                                              \
        }                                                                                                                \
        if (w_ahead_) {              /* MFMA triple, its W pair's successor, ...; the piece in between */                 \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
        } else if ((H) == 0 && g == G0 && (W_FULL1)) {   /* a tile's opening: fragments just ahead of their MFMAs */       \
          __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);                                                             \
        } else {                     /* 2 MFMAs, a read, 2 MFMAs, a read, 2 MFMAs, a piece, 1 MFMA, the other piece, 2 MFMAs */ \
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                                             \
          __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);                                                             \
        }                                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        if (g - G0 == 0) __builtin_amdgcn_s_setprio(2);                                                                  \
        else if (g - G0 == 1) __builtin_amdgcn_s_setprio(1);                                                             \
        else __builtin_amdgcn_s_setprio(0);                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
      }                                                                                                                  \
      if ((H) == 0) issued_prev = (DO_A) ? QF_AIT : 0;                                                                   \
      else issued_prev = (DO_W) ? QF_BIT : 0;                                                                            \
    } while (0)

#define QF_KLOOP_HEAD(PIECE)                                                                                             \
    QF_PHASE(PIECE, 0, 0, true, true, false, false);                                                                     \
    QF_PHASE(PIECE, 0, 1, false, false, nk > 2 || has_next, nk > 1);                                                     \
    int kt = 1;                                                                                                          \
    for (; kt + 2 < nk; ++kt) {                                                                                          \
      QF_PHASE(PIECE, kt, 0, true, false, false, false);                                                                 \
      QF_PHASE(PIECE, kt, 1, false, false, true, true);                                                                  \
    }                                                                                                                    \
    if (nk > 2) {   /* k-tile nk - 2: A(nk - 1) of this tile, then W(0) of the next tile */                              \
      QF_PHASE(PIECE, kt, 0, true, false, false, false);                                                                 \
      QF_PHASE(PIECE, kt, 1, false, false, has_next, true);                                                              \
      ++kt;                                                                                                              \
    }
/* k-tile nk - 1: A(0) of the next tile */
#define QF_KLOOP_TAIL(PIECE)                                                                                             \
    QF_PHASE(PIECE, kt, 0, has_next, false, false, false);                                                               \
    QF_PHASE(PIECE, kt, 1, false, false, false, false);
