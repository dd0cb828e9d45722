// Planner hub: the post-pass over a finished plan (finalize_rungemms / finish_plan) and build_plan().  Builder: plan_builder.h.
#include "plan_builder.h"

namespace sefd {

// Post-pass over a finished plan: give every RUNGEMM the zero page and mark the ones whose runs are whole, 16-byte aligned
// chunks (then the kernel uses the LDS-DMA loader).  Arena buffers are 256-byte aligned, so only element offsets matter.
void finalize_rungemms(Builder& b, Plan* P) {
  // page 0: 256 zero bytes ; page 1: bf16 (1, 0, 0, ...) for the bias "ones" run of the LDS-DMA WGRAD
  char pages[512] = {0};
  pages[256] = (char)0x80; pages[257] = (char)0x3f;
  Ptr z = b.cst(pages, sizeof(pages));
  for (auto* ops : {&P->fwd, &P->bwd})
    for (Op& op : *ops) {
      if (op.kind != OP_RUNGEMM && op.kind != OP_WGRAD) continue;
      RunGemm& g = op.g;
      g.zero = z;
      fastdiv_make((uint32_t)(g.Tout * g.Fo), &g.div_tf_m, &g.div_tf_s);
      fastdiv_make((uint32_t)g.Fo, &g.div_fo_m, &g.div_fo_s);
      const bool ok = runs_aligned(g, op.kind == OP_WGRAD);
      g.flags = (g.flags & ~kRunAligned) | (ok ? kRunAligned : 0);
      if (op.kind == OP_RUNGEMM) {
        const bool ya = g.ydt == DT_BF16 && g.N % 8 == 0 && g.y_off % 8 == 0 && g.y_fstride % 8 == 0 && g.y_tstride % 8 == 0 &&
                        g.y_bstride % 8 == 0 && (g.y.off % 16) == 0;
        g.flags = (g.flags & ~kRunYAligned) | (ya ? kRunYAligned : 0);
      }
      if (!enc0_accepts(g, op.kind == OP_WGRAD) && P->error.empty()) P->error = "first-layer descriptor (kRunEnc0 / kRunDyFromBn) without a kernel";
    }
  // Wide-tile kernel (cgemm256.hip) for the bf16 layers that carry the FLOPs: N a multiple of 256, LDS-DMA-able runs, enough rows.
  // Its weights are packed K-tile major (kRunWTile32): a property of the packed BUFFER, so it is chosen only when every GEMM
  // that reads the buffer qualifies, and the PACK table of the matrix is permuted here, once.  Knob CG256=0: 128 x 128 kernel
  // everywhere (A/B runs).
  {
    const bool wide = tune_on("CG256");
    const bool minm_set = tune_has("CG256_MINM");
    const int wide_minm = (int)tune_int("CG256_MINM", 4096);
    // ... and enough 256 x 256 tiles to occupy the chip: the projection's input gradient (M = B*T = 15 456, N = 256: 61 tiles on 256 CUs) ran
    // 65 us on the wide kernel; as 242 workgroups of the 128-row kernel it fills the chip: 33 us.  Only up to K = 1024: DCCRN-large's few-tile
    // GEMMs have K = 2048 and lost 0.75 ms per step on the 128-row kernel.  (Tests that lower MINM run small cases on purpose.)
    const int wide_mintiles = minm_set ? 0 : 100;          // 50 / 200 tiles measure the same (profiles/r04_tuning_notes.md)
    std::map<int64_t, bool> elig;                            // weight buffer offset -> every reader (either phase) qualifies
    std::vector<Op*> all;
    for (auto* ops : {&P->fwd, &P->bwd})
      for (Op& op : *ops) all.push_back(&op);
    for (Op* op : all) {
      if (op->kind != OP_RUNGEMM || op->g.w.arena != A_WS) continue;
      const RunGemm& g = op->g;
      const bool e = wide && (g.flags & kRunAligned) && g.xdt == DT_BF16 && g.Npad % 256 == 0 && g.ldw % 64 == 0 && g.M >= wide_minm && g.n2 == 0 &&
                     ((((g.M + 255) / 256) * (int64_t)(g.Npad / 256) >= wide_mintiles && (g.ldw >= 256 || minm_set)) || g.ldw > 1024);
      // (... and at least four 64-deep K tiles: the layer-1 LSTM input GEMMs of the chunked forward - M 7 744, N 1024, K 128, 124 tiles - are all prologue and
      //  epilogue on the persistent 256 x 256 tile: 32 us each against 18 us on the 128-row kernel, round 6; the tests that lower MINM run small cases on purpose)
      auto it = elig.find(g.w.off);
      if (it == elig.end()) elig[g.w.off] = e; else it->second = it->second && e;
    }
    for (auto& kv : elig) {
      if (!kv.second) continue;
      const RunGemm* g = nullptr;
      for (Op* op : all) if (op->kind == OP_RUNGEMM && op->g.w.arena == A_WS && op->g.w.off == kv.first) { g = &op->g; break; }
      bool done = false;
      for (Op* po : all) {
        if (po->kind != OP_PACK || po->pack.width != 1 || po->pack.dst.arena != A_WS || po->pack.dst.off != kv.first) continue;
        if (!g || po->pack.n != (int64_t)g->Npad * g->ldw) break;
        int32_t* tab = reinterpret_cast<int32_t*>(P->consts.data() + po->pack.tab.off);
        std::vector<int32_t> old(tab, tab + po->pack.n);
        for (int n = 0; n < g->Npad; ++n)
          for (int k = 0; k < g->ldw; ++k) tab[w_index(kRunWTile32, g->ldw, g->Npad, n, k)] = old[(size_t)n * g->ldw + k];
        done = true;
        break;
      }
      if (done)
        for (Op* op : all) if (op->kind == OP_RUNGEMM && op->g.w.arena == A_WS && op->g.w.off == kv.first) op->g.flags |= kRunWTile32;
    }
  }
  if (tune_has("DUMP_GEMMS")) {                          // planner debugging: every GEMM descriptor of the plan on stderr
    int ph = 0;
    for (auto* ops : {&P->fwd, &P->bwd}) {
      int i = 0;
      for (Op& op : *ops) {
        if (op.kind == OP_RUNGEMM || op.kind == OP_WGRAD) {
          const RunGemm& g = op.g;
          fprintf(stderr, "%s ph%d op%d tag%d M=%d Tout=%d Fo=%d N=%d Npad=%d ldw=%d flags=%d xdt=%d ydt=%d n2=%d nsplit=%d\n", op.kind == OP_RUNGEMM ? "RUNGEMM" : "WGRAD", ph, i,
                  op.tag, g.M, g.Tout, g.Fo, g.N, g.Npad, g.ldw, g.flags, g.xdt, g.ydt, g.n2, g.nsplit);
          for (int s = 0; s < 2; ++s)
            if (g.x[s].arena >= 0) fprintf(stderr, "    src%d bstride=%lld tstride=%d base=%d rowlen=%d fstride=%d Tin=%d\n", s, (long long)g.bstride[s], g.tstride[s], g.base[s], g.rowlen[s], g.fstride[s], g.Tin[s]);
          for (int s = 0; s < g.nseg; ++s) fprintf(stderr, "    seg%d src=%d dt=%d off=%d len=%d koff=%d\n", s, g.seg[s].src, g.seg[s].dt, g.seg[s].off, g.seg[s].len, g.seg[s].koff);
        }
        ++i;
      }
      ++ph;
    }
  }
  // weight repacking: one launch per phase instead of one per matrix (71 launches of ~5 us in a DCCRN step)
  for (auto* ops : {&P->fwd, &P->bwd}) {
    std::vector<Pack> packs;
    std::vector<Op> rest;
    // The first encoder layer on the spectrum (kRunEnc0) keeps its own two tiny PACK launches (2 048 + 32 elements) on the main stream: as part of the
    // phase's PACKMULTI (48 us on the second stream, joined by the first GEMM) it held the first layer back until 70 us into the step although the STFT
    // in front of it ends at 17 us (profiles/r06_timeline.txt); the join moves to the second layer's GEMM
    int64_t own_w = -1, own_b = -1;
    for (Op& op : *ops)
      if (op.kind == OP_RUNGEMM && (op.g.flags & kRunEnc0)) { own_w = op.g.w.off; own_b = op.g.bias.arena >= 0 ? op.g.bias.off : -1; break; }
    for (Op& op : *ops) {
      const bool own = op.kind == OP_PACK && op.pack.dst.arena == A_WS && (op.pack.dst.off == own_w || op.pack.dst.off == own_b);
      if (op.kind == OP_PACK && !own) packs.push_back(op.pack); else rest.push_back(op);
    }
    if (packs.size() < 2) continue;
    Op m;
    std::memset(&m, 0, sizeof(m));
    m.kind = OP_PACKMULTI;
    m.tag = 1;
    m.packm.entries = b.cst(packs.data(), (int64_t)packs.size() * sizeof(Pack));
    m.packm.count = (int32_t)packs.size();
    rest.insert(rest.begin(), m);
    ops->swap(rest);
  }
  // Training plans: both phases' packs ride the second stream during the forward phase (they read only parameters; the backward's 57 us
  // pass sat in the serial loss section, the forward's in front of the STFT).  The forward packs are issued first and joined by the first
  // op that reads a packed matrix; the backward packs are issued right after that op (one launch of both slowed the STFT / spectrum
  // kernels next to it and delayed the first GEMM by 55 us).  Knob PACK_EARLY=0 keeps one launch per phase at its head.
  if (tune_on("PACK_EARLY") && !P->fwd.empty() && !P->bwd.empty() &&
      P->fwd[0].kind == OP_PACKMULTI && P->bwd[0].kind == OP_PACKMULTI) {
    P->fwd[0].lane = 2;
    size_t first = 0;
    for (size_t i = 1; i < P->fwd.size(); ++i) {
      Op& op = P->fwd[i];
      if (op.lane != 0) continue;
      if (op.kind == OP_RUNGEMM && (op.g.flags & kRunEnc0)) continue;                     // reads its own PACK launches, not the PACKMULTI's output
      if (op.kind == OP_RUNGEMM || op.kind == OP_LSTM_FWD || op.kind == OP_WGRAD) { op.join = 1; first = i; break; }
    }
    if (first > 0) {
      Op m = P->bwd[0];
      m.lane = 2;
      P->bwd.erase(P->bwd.begin());
      P->fwd.insert(P->fwd.begin() + first + 1, m);
    } else {
      P->fwd[0].lane = 0;
    }
  }
  // SyncBN (cfg.bn_world > 1): every training-mode BN_FINALIZE becomes "publish this rank's sums" + "statistics from the
  // all-reduced sums" with a sync point in between; every BN_BWD_FINALIZE is followed by a sync point on its totals.
  // ComplexBatchNorm: both CBN_FINALIZE and CBN_BWD_FINALIZE become such a pair around fp64 totals (5 and 6 sums per channel pair).
  // Counts become global: every descriptor that carries a BatchNorm count (BN_FINALIZE, BN_BWD_APPLY, the kRunDyFromBn WGRAD) is scaled here;
  // of the CBN descriptors only the finalize ops read theirs.
  // The caller (models.py / hostsim tests) runs the op ranges between sync points and all-reduces.
  const int world = P->cfg.bn_world;
  if (world > 1 && P->cfg.training) {
    int k = 0;
    for (int phase = 0; phase < 2; ++phase) {
      std::vector<Op>& ops = phase == 0 ? P->fwd : P->bwd;
      std::vector<Op> out;
      for (Op op : ops) {
        if (op.kind == OP_BN_FINALIZE && op.bnf.nblk >= 0) {
          op.bnf.totals = b.ws("syncbn.tot" + std::to_string(k++), (int64_t)2 * op.bnf.C * 2, DT_F32);   // 2*C doubles
          op.bnf.mode = 1;
          out.push_back(op);
          P->syncs.push_back(SyncPoint{phase, (int32_t)out.size() - 1, op.bnf.totals, 2 * (int64_t)op.bnf.C, 1});
          op.bnf.mode = 2;
          op.bnf.count *= world;
          out.push_back(op);
        } else if (op.kind == OP_BN_BWD_FINALIZE) {
          out.push_back(op);
          P->syncs.push_back(SyncPoint{phase, (int32_t)out.size() - 1, op.bnb.totals, 2 * (int64_t)op.bnb.r.C, 0});
        } else if (op.kind == OP_BN_BWD_APPLY) {
          op.bnb.count *= world;
          out.push_back(op);
        } else if ((op.kind == OP_CBN_FINALIZE && op.cbf.training) || op.kind == OP_CBN_BWD_FINALIZE) {
          const bool fwd = op.kind == OP_CBN_FINALIZE;
          const int h = fwd ? op.cbf.C / 2 : op.cbb.C / 2, ns = fwd ? 5 : 6;
          const Ptr tot = b.ws("syncbn.ctot" + std::to_string(k++), (int64_t)ns * h * 2, DT_F32);     // ns*h doubles
          if (fwd) { op.cbf.totals = tot; op.cbf.mode = 1; } else { op.cbb.totals = tot; op.cbb.mode = 1; }
          out.push_back(op);
          P->syncs.push_back(SyncPoint{phase, (int32_t)out.size() - 1, tot, (int64_t)ns * h, 1});
          if (fwd) { op.cbf.mode = 2; op.cbf.count *= world; } else { op.cbb.mode = 2; op.cbb.count *= world; }
          out.push_back(op);
        } else if (op.kind == OP_WGRAD && (op.g.flags & kRunDyFromBn)) {
          op.g.bnb_inv_count /= (float)world;       // the BatchNorm backward fused into enc0's weight gradient divides the all-reduced totals
          out.push_back(op);
        } else {
          out.push_back(op);
        }
      }
      ops.swap(out);
    }
  }
}

// Plan epilogue: the post-pass, then the arena sizes (nparam trainable elements, nstate BatchNorm buffer elements; at least one each)
void finish_plan(Builder& b, Plan* P, int64_t nparam, int64_t nstate) {
  finalize_rungemms(b, P);
  P->arena_bytes[A_WS] = b.ws_off;
  P->arena_bytes[A_PARAM] = std::max<int64_t>(nparam, 1) * 4;
  P->arena_bytes[A_GRAD] = std::max<int64_t>(nparam, 1) * 4;
  P->arena_bytes[A_STATE] = std::max<int64_t>(nstate, 1) * 4;
  P->arena_bytes[A_CONST] = (int64_t)P->consts.size();
  P->arena_bytes[A_IO] = b.io_off;
}

Plan* build_plan(const ModelConfig& cfg) {
  if (cfg.model == 13) return build_torchistft_adj_plan(cfg);
  if (cfg.model == 12) return build_torchstft_adj_plan(cfg);
  if (cfg.model == 11) return build_clstm_plan(cfg);
  if (cfg.model == 10) return build_cbn_plan(cfg);
  if (cfg.model == 9) return build_convlayer_plan(cfg);
  if (cfg.model == 8) return build_convistft_plan(cfg);
  if (cfg.model == 7) return build_convstft_plan(cfg);
  if (cfg.model == 6) return build_seq_plan(cfg);
  if (cfg.model == 5) return build_torchistft_plan(cfg);
  if (cfg.model == 4) return build_torchstft_plan(cfg);
  if (cfg.model == 3) return build_fsn_plan(cfg);
  return cfg.model == 2 ? build_frontend_plan(cfg) : (cfg.model == 1 ? build_crn_plan(cfg) : build_dccrn_plan(cfg));
}

}  // namespace sefd
