// sched_host.cpp — the multi-GPU rounds' schedules and cost model
// (sched_host.h): the geometry, the five schedule builders, the stream rules,
// the discrete-event model and the host-only entry points of fedagg_comm.h.
// Plain C++17: no HIP header, no RCCL header, no device.  Of libfedagg.so it
// calls fa_plan_build_host_elem and fa_chain_levels (plan_host.cpp, as HIP-free).

#include "sched_host.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>

namespace fa_sched __attribute__((visibility("hidden"))) {
using fa::set_err;

int check_round_args(const char* who, int mode, int* nchunks, int xchg, int root, int nranks) {
  if (mode != FA_MODE_SHARDED && mode != FA_MODE_STRIPED && mode != FA_MODE_CHAINED &&
      mode != FA_MODE_BLOCKED)
    return set_err(FA_E_INVAL, "%s: mode %d", who, mode);
  if (*nchunks == 0) *nchunks = mode == FA_MODE_STRIPED ? kStripeChunks : 8;
  if (*nchunks < 1 || *nchunks > FA_COMM_MAX_CHUNKS)
    return set_err(FA_E_INVAL, "%s: nchunks=%d", who, *nchunks);
  if (xchg != FA_XCHG_REDUCE && xchg != FA_XCHG_RS_GATHER)
    return set_err(FA_E_INVAL, "%s: exchange %d", who, xchg);
  if (root >= nranks) return set_err(FA_E_INVAL, "%s: root=%d", who, root);
  return FA_OK;
}

// ------------------------------------------------------------- geometry ----
int make_geo(int nranks, int rank, const int* counts, const fa_seg* seg32, int nseg32,
             int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
             unsigned flags, const char* who, Geo* g, int elem) {
  if (elem != FA_ELEM_F32 && elem != FA_ELEM_F16 && elem != FA_ELEM_BF16)
    return set_err(FA_E_INVAL, "%s: elem=%d", who, elem);
  if (!counts) return set_err(FA_E_INVAL, "%s: counts is NULL", who);
  if (nranks < 1 || rank < 0 || rank >= nranks)
    return set_err(FA_E_INVAL, "%s: rank %d of %d", who, rank, nranks);
  if (!(flags & FA_PLAN_GAPS_ARE_PADDING))
    return set_err(FA_E_INVAL,
                   "%s: the layout must allow writes to its padding "
                   "(FA_PLAN_GAPS_ARE_PADDING): exchanges span it",
                   who);
  g->nranks = nranks;
  g->rank = rank;
  g->counts.assign(counts, counts + nranks);
  g->first.clear();
  g->n_total = 0;
  g->nmax = 0;
  for (int r = 0; r < nranks; ++r) {
    if (counts[r] < 0) return set_err(FA_E_INVAL, "%s: counts[%d]=%d", who, r, counts[r]);
    g->first.push_back(g->n_total);
    g->n_total += counts[r];
    g->nmax = std::max(g->nmax, counts[r]);
  }
  if (g->n_total < 1 || g->n_total > FA_MAX_CLIENTS)
    return set_err(FA_E_RANGE, "%s: %d clients in total", who, g->n_total);
  g->n_local = counts[rank];
  g->lo_slot = g->first[rank];
  g->f32_numel = f32_numel;
  g->i64_numel = i64_numel;
  g->flags = flags;
  g->elem = elem;
  // (FA_ELEM_F32: fa_plan_build_host's table)
  fa_plan_info info{};
  int rc = fa_plan_build_host_elem(seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, 0, flags,
                                   elem, nullptr, 0, &info);
  if (rc) return rc;
  std::vector<fa_tile_desc> tiles(std::max(1, info.ntiles));
  rc = fa_plan_build_host_elem(seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, 0, flags,
                               elem, tiles.data(), info.ntiles, &info);
  if (rc) return rc;
  tiles.resize(info.ntiles);
  g->t32.clear();
  g->t64.clear();
  for (const fa_tile_desc& t : tiles) (t.kind >= 4 ? g->t64 : g->t32).push_back(t);
  std::sort(g->t32.begin(), g->t32.end(),
            [](const fa_tile_desc& a, const fa_tile_desc& b) { return a.start < b.start; });
  return FA_OK;
}

int check_round_elem(const char* who, int elem, int mode, int weighted) {
  if (elem == FA_ELEM_F32) return FA_OK;
  if (elem != FA_ELEM_F16 && elem != FA_ELEM_BF16)
    return set_err(FA_E_INVAL, "%s: elem=%d", who, elem);
  if (mode != FA_MODE_STRIPED)
    return set_err(FA_E_INVAL,
                   "%s: mode %d on a 16-bit bucket: only the striped round (FA_MODE_STRIPED) "
                   "runs on fp16 / bf16 buckets (the other forms move fp32 sums or cascade state)",
                   who, mode);
  if (weighted)
    return set_err(FA_E_INVAL,
                   "%s: a weighted round on a 16-bit bucket: the pre-multiplied rows are fp32 "
                   "values, which a 16-bit exchange cannot carry",
                   who);
  return FA_OK;
}

// FA_ROUND_CHAIN16: the chained round on a 16-bit bucket, mean or weighted;
// nothing else takes the bit.  Without a bit: check_round_elem.
int check_round_opts(const char* who, int elem, int mode, int weighted, unsigned ropts) {
  if (ropts & ~(unsigned)FA_ROUND_CHAIN16)
    return set_err(FA_E_INVAL, "%s: unknown round options 0x%x", who, ropts);
  if (!(ropts & FA_ROUND_CHAIN16)) return check_round_elem(who, elem, mode, weighted);
  if (elem != FA_ELEM_F16 && elem != FA_ELEM_BF16)
    return set_err(FA_E_INVAL,
                   "%s: FA_ROUND_CHAIN16 with elem=%d: the option names the chained round on an "
                   "fp16 / bf16 bucket (an fp32 bucket chains without it)",
                   who, elem);
  if (mode != FA_MODE_CHAINED)
    return set_err(FA_E_INVAL,
                   "%s: FA_ROUND_CHAIN16 with mode %d: the option names the chained round "
                   "(FA_MODE_CHAINED) only",
                   who, mode);
  return FA_OK;
}

namespace {

// k contiguous groups of sorted tiles with equal shares of the elements, cut
// only before a vector tile on a 256-B boundary (`align` elements: 64 fp32,
// 128 fp16 / bf16); exactly k groups, trailing ones may be empty.  Group g =
// tiles [cut[g], cut[g+1]).
void cut_tiles(const std::vector<fa_tile_desc>& t, int k, std::vector<size_t>* cut,
               int align = 64) {
  int64_t total = 0;
  for (const fa_tile_desc& x : t) total += x.count;
  cut->assign(1, 0);
  int64_t acc = 0;
  for (size_t i = 0; i < t.size(); ++i) {
    const int c = (int)cut->size();
    if (c < k && i > 0 && acc >= total * c / k && t[i].kind == 0 && t[i].start % align == 0)
      cut->push_back(i);
    acc += t[i].count;
  }
  while ((int)cut->size() < k + 1) cut->push_back(t.size());
}

// Group g's bucket range: [lo[g], lo[g+1]) with lo[0] = 0 and lo[k] =
// f32_numel — the groups tile the whole bucket (padding included).
std::vector<int64_t> cut_bounds(const std::vector<fa_tile_desc>& t,
                                const std::vector<size_t>& cut, int64_t f32_numel) {
  const int k = (int)cut.size() - 1;
  std::vector<int64_t> lo(k + 1, f32_numel);
  lo[0] = 0;
  for (int g = 1; g < k; ++g) lo[g] = cut[g] < t.size() ? t[cut[g]].start : f32_numel;
  return lo;
}

// ------------------------------------------------------------- schedules ---
struct Sched {
  std::vector<fa_xfer> ops;
  int step = 0;
  void add(int op, int peer, int src, int si, int dst, int di, int64_t off, int64_t cnt,
           int chunk = -1, int row0 = 0, int nrows = 0) {
    fa_xfer x;
    memset(&x, 0, sizeof x);
    x.step = step;
    x.op = op;
    x.peer = peer;
    x.chunk = chunk;
    x.src = src;
    x.src_index = si;
    x.dst = dst;
    x.dst_index = di;
    x.offset = off;
    x.count = cnt;
    x.row0 = row0;
    x.nrows = nrows;
    ops.push_back(x);
  }
  void next() { ++step; }
};

// The int64 keys (num_batches_tracked) of every client, gathered raw and
// reduced exactly by the result ranks; with `tails`, the fp32 scalar columns
// (ILP-4 tails, M==1) too.  stack -> all-gather -> (result ranks) reduce.
void sched_raw_gather(Sched* S, const Geo& g, int64_t t32_width, bool tails, bool result) {
  const bool i64 = !g.t64.empty();
  if (!i64 && !(tails && t32_width)) return;
  if (g.n_local > 0) S->add(FA_X_K_STACK, -1, FA_B_CLIENT, -1, FA_B_STACK, -1, 0, 0, -1,
                            g.lo_slot, g.n_local);
  S->next();
  if (tails && t32_width)
    S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 0, FA_B_GATHER, 0, 0, (int64_t)g.nmax * t32_width);
  if (i64)
    S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 1, FA_B_GATHER, 1, 0,
           (int64_t)g.nmax * g.i64_numel);
  S->next();
  if (result) S->add(FA_X_K_TAILS, -1, FA_B_GATHER, -1, FA_B_OUT, -1, 0, 0, -1, 0, g.n_total);
  S->next();
}

// e1: chunked partial sums + RCCL reduce (or reduce-scatter + gather).
void sched_sharded(const Geo& g, const std::vector<std::pair<int64_t, int64_t>>& range, int xchg,
                   int root, bool weighted, Sched* S) {
  const int me = g.rank, W = g.nranks;
  const bool result = root < 0 || root == me;
  for (size_t c = 0; c < range.size(); ++c) {
    const int64_t lo = range[c].first, L = range[c].second - lo;
    if (g.n_local > 0)
      S->add(FA_X_K_SUM, -1, FA_B_CLIENT, -1, FA_B_PARTIAL, -1, lo, L, (int)c, g.lo_slot,
             g.n_local);
    else
      S->add(FA_X_K_ZERO, -1, FA_B_NONE, -1, FA_B_PARTIAL, -1, lo, L, (int)c);
    S->next();
    const int64_t q = xchg == FA_XCHG_RS_GATHER ? L / W : 0;
    if (q > 0) {
      // in place: rank r's share of the sum lands at partial[lo + r*q, +q)
      S->add(FA_X_REDUCE_SCATTER, -1, FA_B_PARTIAL, -1, FA_B_PARTIAL, -1, lo, q * W);
      S->next();
      if (root < 0)
        S->add(FA_X_ALLGATHER, -1, FA_B_PARTIAL, -1, FA_B_OUT, -1, lo, q * W);
      else
        S->add(FA_X_GATHER, root, FA_B_PARTIAL, -1, result ? FA_B_OUT : FA_B_NONE, -1, lo,
               q * W);
    }
    const int64_t rlo = lo + q * W, rl = L - q * W;  // (all of it for a plain reduce)
    if (rl > 0) {
      if (root < 0)
        S->add(FA_X_ALLREDUCE, -1, FA_B_PARTIAL, -1, FA_B_OUT, -1, rlo, rl);
      else
        S->add(FA_X_REDUCE, root, FA_B_PARTIAL, -1, result ? FA_B_OUT : FA_B_PARTIAL, -1, rlo,
               rl);
    }
    S->next();
    if (result && !weighted) S->add(FA_X_K_DIV, -1, FA_B_OUT, -1, FA_B_OUT, -1, lo, L, (int)c);
    S->next();
  }
  sched_raw_gather(S, g, 0, false, result);
}

// e2: column stripes, cut into column chunks; every peer in one group per
// chunk (r06, VERDICT r05 next 1: r02-r05 ran one RCCL group per partner, so
// a rank used one of its xGMI links at a time).  clo[r][c .. c+1]: chunk c of
// rank r's stripe.  Step 2 + j carries, in ONE group, chunk j's client
// exchange with every peer and the finished chunk j - 2 to the result ranks,
// and — on the caller's stream, concurrent with that group — the stripe
// reduce of chunk j - 1, whose rows arrived in the previous step's group
// (the executor starts a compute-stream kernel that reads exchanged data
// after the exchanges of the steps BEFORE its own: reads_exchanged below).
// Per pair, the sender posts its client rows then its result chunk and the
// receiver its receives in the same order (RCCL matches a pair's sends and
// receives in posting order).  Weighted: the rows sent are the local
// clients' pre-multiplied values (FA_X_K_SCALE into WSTAGE, step 0).
void sched_striped(const Geo& g, const std::vector<std::vector<int64_t>>& clo, int root,
                   bool weighted, Sched* S) {
  const int me = g.rank, W = g.nranks;
  const int C = (int)clo[0].size() - 1;
  const bool result = root < 0 || root == me;
  const bool i64 = !g.t64.empty();
  auto len = [&](int r, int c) { return clo[r][c + 1] - clo[r][c]; };
  // step 0: the int64 keys stacked; weighted: the local clients' values
  // outside this rank's stripe (what the peers receive) pre-multiplied
  if (i64 && g.n_local > 0)
    S->add(FA_X_K_STACK, -1, FA_B_CLIENT, -1, FA_B_STACK, -1, 0, 0, -1, g.lo_slot, g.n_local);
  const int64_t mlo = clo[me][0], mhi = clo[me][C];
  if (weighted && g.n_local > 0) {
    if (mlo > 0)
      S->add(FA_X_K_SCALE, -1, FA_B_CLIENT, -1, FA_B_WSTAGE, -1, 0, mlo, -1, 0, g.n_local);
    if (mhi < g.f32_numel)
      S->add(FA_X_K_SCALE, -1, FA_B_CLIENT, -1, FA_B_WSTAGE, -1, mhi, g.f32_numel - mhi, -1, 0,
             g.n_local);
  }
  S->next();
  // step 1: the int64 keys of every rank (a few bytes)
  if (i64)
    S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 1, FA_B_GATHER, 1, 0, (int64_t)g.nmax * g.i64_numel);
  S->next();
  const int src = weighted ? FA_B_WSTAGE : FA_B_CLIENT;
  for (int j = 0; j <= C + 1; ++j) {
    for (int q = 1; q < W; ++q) {  // peers in a rotated order: rank me + q first
      const int r = (me + q) % W;
      if (j < C) {
        if (len(r, j) > 0)
          for (int k = 0; k < g.n_local; ++k)
            S->add(FA_X_SEND, r, src, k, FA_B_NONE, -1, clo[r][j], len(r, j), j);
        if (len(me, j) > 0)
          for (int k = 0; k < g.counts[r]; ++k)
            S->add(FA_X_RECV, r, FA_B_NONE, -1, FA_B_RECV, g.first[r] + k, clo[me][j],
                   len(me, j), j);
      }
      const int c = j - 2;
      if (c >= 0 && c < C) {
        if (len(me, c) > 0 && (root < 0 || root == r))
          S->add(FA_X_SEND, r, result ? FA_B_OUT : FA_B_STRIPE, -1, FA_B_NONE, -1, clo[me][c],
                 len(me, c), c);
        if (len(r, c) > 0 && result)
          S->add(FA_X_RECV, r, FA_B_NONE, -1, FA_B_OUT, -1, clo[r][c], len(r, c), c);
      }
    }
    const int k = j - 1;
    if (k >= 0 && k < C && len(me, k) > 0)
      S->add(FA_X_K_STRIPE, -1, FA_B_RECV, -1, result ? FA_B_OUT : FA_B_STRIPE, -1, clo[me][k],
             len(me, k), k, 0, g.n_total);
    S->next();
  }
  if (i64 && result)
    S->add(FA_X_K_TAILS, -1, FA_B_GATHER, -1, FA_B_OUT, -1, 0, 0, -1, 0, g.n_total);
  S->next();
}

// A 16-bit round (FA_ROUND_CHAIN16): CLIENT, OUT, FIN and the stacked scalar
// columns hold 16-bit elements, the STATE planes fp32.  Weighted, the chain
// kernels multiply by the local weights and the scalar columns travel raw, so
// the result ranks need every rank's weights: one more all-gather (STACK /
// GATHER index 2, nmax floats per rank) in the scalar columns' group.
void sched_chained(const Geo& g, const ChainGeo& cg, int root, bool weighted, Sched* S) {
  const int me = g.rank, F = cg.finisher;
  const bool result = root < 0 || root == me;
  // the raw scalar columns first: their gather overlaps the chain
  const int64_t C = (int64_t)cg.range.size();
  const bool i64 = !g.t64.empty();
  if (i64 || cg.t32_width) {
    if (g.n_local > 0)
      S->add(FA_X_K_STACK, -1, FA_B_CLIENT, -1, FA_B_STACK, -1, 0, 0, -1, g.lo_slot, g.n_local);
    S->next();
    if (cg.t32_width)
      S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 0, FA_B_GATHER, 0, 0, (int64_t)g.nmax * cg.t32_row);
    if (i64)
      S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 1, FA_B_GATHER, 1, 0,
             (int64_t)g.nmax * g.i64_numel);
    if (weighted && g.elem != FA_ELEM_F32 && cg.t32_width)
      S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 2, FA_B_GATHER, 2, 0, (int64_t)g.nmax);
    S->next();
  }
  if (me <= F) {
    const bool pred = me > 0 && cg.lev_in, succ = me < F && cg.lev_out;
    auto planes = [&](int op, int peer, unsigned lev, int64_t c) {
      for (int l = 0; l < 4; ++l)
        if (lev & (1u << l)) {
          const int64_t lo = cg.range[c].first, L = cg.range[c].second - lo;
          if (op == FA_X_SEND) S->add(op, peer, FA_B_STATE, l, FA_B_NONE, -1, lo, L, (int)c);
          else S->add(op, peer, FA_B_NONE, -1, FA_B_STATE, l, lo, L, (int)c);
        }
    };
    const int fin = me < F ? FA_B_STATE : (result ? FA_B_OUT : FA_B_FIN);
    for (int64_t c = 0; c <= C; ++c) {
      if (succ && c > 0) planes(FA_X_SEND, me + 1, cg.lev_out, c - 1);
      if (pred && c < C) planes(FA_X_RECV, me - 1, cg.lev_in, c);
      S->next();
      if (c < C && g.n_local > 0) {
        const int64_t lo = cg.range[c].first, L = cg.range[c].second - lo;
        S->add(FA_X_K_CHAIN, -1, pred ? FA_B_STATE : FA_B_NONE, -1, fin, -1, lo, L, (int)c,
               g.lo_slot, g.n_local);
      }
      S->next();
    }
  } else {
    S->step += 2 * (int)(C + 1);
  }
  // the finished vector columns to the result ranks
  if (C > 0) {
    const int64_t lo = cg.range[0].first, L = cg.range[C - 1].second - lo;
    if (root < 0) {
      S->add(FA_X_BCAST, F, me == F ? FA_B_OUT : FA_B_NONE, -1, FA_B_OUT, -1, lo, L);
    } else if (root != F) {
      if (me == F) S->add(FA_X_SEND, root, FA_B_FIN, -1, FA_B_NONE, -1, lo, L);
      if (me == root) S->add(FA_X_RECV, F, FA_B_NONE, -1, FA_B_OUT, -1, lo, L);
    }
  }
  S->next();
  if (result && (i64 || cg.t32_width))
    S->add(FA_X_K_TAILS, -1, FA_B_GATHER, -1, FA_B_OUT, -1, 0, 0, -1, 0, g.n_total);
  S->next();
}

// Blocked: block sums where they lie, spanning blocks' partials relayed
// through the stripe owners, block sums to the owners, fold, results out.
void sched_blocked(const Geo& g, const ChainGeo& cg, const BlockGeo& bg, int root, Sched* S) {
  const int me = g.rank, W = g.nranks;
  const bool result = root < 0 || root == me;
  const bool i64 = !g.t64.empty();
  auto w_of = [&](int s) { return bg.shi[s] - bg.slo[s]; };
  const bool vec = !cg.range.empty();  // a layout of scalar columns only has no blocks
  // step 0: the partial a neighbour waits for, alone
  if ((i64 || cg.t32_width) && g.n_local > 0)
    S->add(FA_X_K_STACK, -1, FA_B_CLIENT, -1, FA_B_STACK, -1, 0, 0, -1, g.lo_slot, g.n_local);
  if (vec && bg.tail_piece >= 0) {
    const int i = bg.tail_piece;
    S->add(FA_X_K_PART, -1, FA_B_PIN, -1, FA_B_TAILP, 0, 0, 0, -1, bg.s0[i],
           g.lo_slot + g.n_local - bg.s0[i]);
  }
  S->next();
  // step 1: raw columns gathered; each spanning partial split into stripes,
  // to its holder directly (the starter's and the holder's own stripes) or
  // to the stripe's owner
  if (cg.t32_width)
    S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 0, FA_B_GATHER, 0, 0, (int64_t)g.nmax * cg.t32_row);
  if (i64)
    S->add(FA_X_ALLGATHER, -1, FA_B_STACK, 1, FA_B_GATHER, 1, 0, (int64_t)g.nmax * g.i64_numel);
  for (int i = 0; i < bg.P; ++i) {
    const int r1 = bg.starter[i], r2 = bg.holder[i];
    if (r1 == r2) continue;
    for (int s = 0; s < W; ++s) {
      const int64_t w = w_of(s);
      if (w == 0) continue;
      const int64_t off = bg.slo[s];
      const bool direct = s == r1 || s == r2;
      if (me == r1) S->add(FA_X_SEND, direct ? r2 : s, FA_B_TAILP, 0, FA_B_NONE, -1, off, w);
      if (direct && me == r2) S->add(FA_X_RECV, r1, FA_B_NONE, -1, FA_B_PIN, 0, off, w);
      if (!direct && me == s) S->add(FA_X_RECV, r1, FA_B_NONE, -1, FA_B_RELAY, r1, off, w);
    }
  }
  // the local block sums on the compute stream, behind the partial's
  // scatter and overlapping it and the forwarding step (which reads only
  // relayed data)
  for (int i = 0; i < bg.P && vec; ++i)
    if (bg.bsum_slot[i] >= 0)
      S->add(FA_X_K_BLOCK, -1, FA_B_CLIENT, -1, FA_B_BSUM, bg.bsum_slot[i], 0, 0, i, bg.s0[i],
             bg.s1[i] - bg.s0[i]);
  S->next();
  // step 2: the owners forward their stripes of the partials
  for (int i = 0; i < bg.P; ++i) {
    const int r1 = bg.starter[i], r2 = bg.holder[i];
    if (r1 == r2) continue;
    for (int s = 0; s < W; ++s) {
      const int64_t w = w_of(s);
      if (w == 0 || s == r1 || s == r2) continue;
      if (me == s) S->add(FA_X_SEND, r2, FA_B_RELAY, r1, FA_B_NONE, -1, bg.slo[s], w);
      if (me == r2) S->add(FA_X_RECV, s, FA_B_NONE, -1, FA_B_PIN, 0, bg.slo[s], w);
    }
  }
  S->next();
  // step 3: the holder finishes the spanning block (or the remainder)
  if (vec && bg.head_piece >= 0) {
    const int i = bg.head_piece;
    S->add(FA_X_K_CONT, -1, FA_B_PIN, -1, FA_B_CONT, bg.plane[i], 0, 0, i, g.lo_slot,
           bg.s1[i] - g.lo_slot);
  }
  S->next();
  // step 4: every piece's stripes to their owners, in piece order
  for (int i = 0; i < bg.P; ++i) {
    const int h = bg.holder[i];
    const bool local = bg.starter[i] == h;
    for (int s = 0; s < W; ++s) {
      const int64_t w = w_of(s);
      if (w == 0 || s == h) continue;
      if (me == h) {
        if (local) S->add(FA_X_SEND, s, FA_B_BSUM, bg.bsum_slot[i], FA_B_NONE, -1, bg.slo[s], w);
        else S->add(FA_X_SEND, s, FA_B_CONT, bg.plane[i], FA_B_NONE, -1, bg.slo[s], w);
      }
      if (me == s) S->add(FA_X_RECV, h, FA_B_NONE, -1, FA_B_BLK, i, bg.slo[s], w);
    }
  }
  S->next();
  // step 5: own pieces into the stripe, then the fold
  const int64_t wme = w_of(me);
  if (vec && wme > 0) {
    for (int i = 0; i < bg.P; ++i) {
      if (bg.holder[i] != me) continue;
      if (bg.bsum_slot[i] >= 0)
        S->add(FA_X_K_COPY, -1, FA_B_BSUM, bg.bsum_slot[i], FA_B_BLK, i, bg.slo[me], wme);
      else
        S->add(FA_X_K_COPY, -1, FA_B_CONT, bg.plane[i], FA_B_BLK, i, bg.slo[me], wme);
    }
    S->add(FA_X_K_FOLD, -1, FA_B_BLK, -1, result ? FA_B_OUT : FA_B_FIN, -1, bg.slo[me], wme, me,
           0, bg.P);
  }
  S->next();
  // step 6: the folded stripes to the result ranks
  for (int s = 0; s < W; ++s) {
    const int64_t w = w_of(s);
    if (w == 0) continue;
    for (int r = 0; r < W; ++r) {
      if (r == s || !(root < 0 || root == r)) continue;
      const bool s_result = root < 0 || root == s;
      if (me == s)
        S->add(FA_X_SEND, r, s_result ? FA_B_OUT : FA_B_FIN, -1, FA_B_NONE, -1, bg.slo[s], w);
      if (me == r) S->add(FA_X_RECV, s, FA_B_NONE, -1, FA_B_OUT, -1, bg.slo[s], w);
    }
  }
  S->next();
  if (result && (i64 || cg.t32_width))
    S->add(FA_X_K_TAILS, -1, FA_B_GATHER, -1, FA_B_OUT, -1, 0, 0, -1, 0, g.n_total);
  S->next();
}

// The chained mode's cut of the layout: vector tiles chunked, scalar fp32
// columns compacted (their bucket index per compact column).
void chain_geo(const Geo& g, int nchunks, ChainGeo* cg, std::vector<fa_tile_desc>* vec,
               std::vector<size_t>* cut, std::vector<fa_tile_desc>* tails,
               std::vector<int64_t>* tidx) {
  vec->clear();
  tails->clear();
  tidx->clear();
  for (const fa_tile_desc& t : g.t32) {
    if (t.kind == 0) {
      vec->push_back(t);
    } else {
      fa_tile_desc c = t;
      c.start = (int64_t)tidx->size();  // compact coordinates
      tails->push_back(c);
      for (int32_t e = 0; e < t.count; ++e) tidx->push_back(t.start + e);
    }
  }
  cg->t32_width = (int64_t)tidx->size();
  cg->t32_row = (cg->t32_width + 63) / 64 * 64;
  cg->range.clear();
  cut_tiles(*vec, nchunks, cut, cut_align(g.elem));
  std::vector<size_t> keep(1, 0);
  for (int c = 0; c < nchunks; ++c) {
    if ((*cut)[c] == (*cut)[c + 1]) continue;
    const fa_tile_desc& a = (*vec)[(*cut)[c]];
    const fa_tile_desc& b = (*vec)[(*cut)[c + 1] - 1];
    cg->range.emplace_back(a.start, b.start + b.count);
    keep.push_back((*cut)[c + 1]);
  }
  *cut = keep;
  cg->finisher = 0;
  for (int r = 0; r < g.nranks; ++r)
    if (g.counts[r] > 0) cg->finisher = r;
  cg->lev_in = fa_chain_levels(g.lo_slot, g.n_total);
  cg->lev_out = fa_chain_levels(g.lo_slot + g.n_local, g.n_total);
}

int rank_of_row(const Geo& g, int i) {
  for (int r = 0; r < g.nranks; ++r)
    if (i >= g.first[r] && i < g.first[r] + g.counts[r]) return r;
  return -1;
}

// The cascade's level step for n rows (fa_reduce's lp: 16 below 2^16 rows).
int cascade_lp(int n) {
  int c = 0;
  while ((1ll << c) < n) ++c;
  return std::max(4, c / 4);
}

// The blocked round's condition from the counts alone: the first cascade
// block (slots [*a, *b)) whose slots lie on more than two of the ranks that
// hold slots (ranks without slots in between do not count), or -1 when every
// block fits.  block_geo and fa_multi_select share it.
int first_wide_block(int nranks, const int* counts, int* a_out, int* b_out) {
  int n = 0;
  std::vector<int> first(nranks);
  for (int r = 0; r < nranks; ++r) {
    first[r] = n;
    n += std::max(0, counts[r]);
  }
  const int Q = 1 << cascade_lp(n);
  for (int i = 0, a = 0; a < n; ++i, a += Q) {
    const int b = std::min(n, a + Q);
    int on = 0;
    for (int r = 0; r < nranks; ++r)
      if (counts[r] > 0 && first[r] < b && first[r] + counts[r] > a) ++on;
    if (on > 2) {
      if (a_out) *a_out = a;
      if (b_out) *b_out = b;
      return i;
    }
  }
  return -1;
}

int block_geo(const Geo& g, const std::vector<fa_tile_desc>& vec, BlockGeo* bg) {
  const int n = g.n_total;
  const int lp = cascade_lp(n);
  {
    int a = 0, b = 0;
    if (first_wide_block(g.nranks, g.counts.data(), &a, &b) >= 0)
      return set_err(FA_E_RANGE,
                     "blocked round: slots %d..%d (one cascade block) lie on more than two "
                     "ranks; use the chained round",
                     a, b - 1);
  }
  bg->lp = lp;
  const int Q = 1 << lp, mask = Q - 1;
  bg->K = n / Q;
  bg->P = bg->K + (n % Q ? 1 : 0);
  bg->s0.clear(); bg->s1.clear(); bg->starter.clear(); bg->holder.clear();
  bg->bsum_slot.clear(); bg->plane.clear();
  bg->tail_piece = bg->head_piece = -1;
  bg->nbsum = 0;
  for (int i = 0; i < bg->P; ++i) {
    const int a = i * Q, b = std::min(n, a + Q);
    // (first_wide_block above: the holder is the next rank holding slots
    // after the starter)
    const int r0 = rank_of_row(g, a), r1 = rank_of_row(g, b - 1);
    bg->s0.push_back(a);
    bg->s1.push_back(b);
    bg->starter.push_back(r0);
    bg->holder.push_back(r1);
    int j = 0;
    if (r0 != r1 && i < bg->K && b < n) {
      j = 1;
      if ((b & (mask << lp)) == 0) j = (b & (mask << (2 * lp))) == 0 ? 3 : 2;
    }
    bg->plane.push_back(j);  // 0: a finishing continuation writes CONT plane 0
    if (r0 == r1) {
      bg->bsum_slot.push_back(r1 == g.rank ? bg->nbsum++ : -1);
    } else {
      bg->bsum_slot.push_back(-1);
      if (r0 == g.rank) bg->tail_piece = i;
      if (r1 == g.rank) bg->head_piece = i;
    }
  }
  // owner stripes over the vector tiles
  std::vector<size_t> cut;
  cut_tiles(vec, g.nranks, &cut);
  bg->slo.assign(g.nranks, 0);
  bg->shi.assign(g.nranks, 0);
  int64_t w = 0;
  for (int s = 0; s < g.nranks; ++s) {
    if (cut[s] == cut[s + 1]) continue;
    bg->slo[s] = vec[cut[s]].start;
    const fa_tile_desc& t = vec[cut[s + 1] - 1];
    bg->shi[s] = t.start + t.count;
    w = std::max(w, bg->shi[s] - bg->slo[s]);
  }
  bg->row = (w + 63) / 64 * 64;
  return FA_OK;
}

// e1 chunk ranges over the whole bucket.
void shard_ranges(const Geo& g, int nchunks, std::vector<size_t>* cut_out,
                  std::vector<std::pair<int64_t, int64_t>>* range) {
  std::vector<size_t> cut;
  cut_tiles(g.t32, nchunks, &cut);
  const std::vector<int64_t> lo = cut_bounds(g.t32, cut, g.f32_numel);
  range->clear();
  cut_out->assign(1, 0);
  for (int c = 0; c < nchunks; ++c) {
    if (cut[c] == cut[c + 1]) continue;
    range->emplace_back(lo[c], lo[c + 1]);
    cut_out->push_back(cut[c + 1]);
  }
  if (!range->empty()) range->back().second = g.f32_numel;
}

}  // namespace

int build_round(RoundGeo* p, int nchunks, std::vector<fa_tile_desc>* vec_out,
                std::vector<size_t>* cut_out, std::vector<fa_tile_desc>* tails_out,
                std::vector<int64_t>* tidx_out) {
  const Geo& g = p->g;
  if (p->mode == FA_MODE_SHARDED) {
    shard_ranges(g, nchunks, cut_out, &p->range);
  } else if (p->mode == FA_MODE_STRIPED) {
    // stripes, then each stripe's tiles cut into nchunks column chunks
    std::vector<size_t> cut;
    cut_tiles(g.t32, g.nranks, &cut, cut_align(g.elem));
    p->lo = cut_bounds(g.t32, cut, g.f32_numel);
    p->nchunks = nchunks;
    p->clo.assign(g.nranks, std::vector<int64_t>());
    cut_out->clear();
    for (int r = 0; r < g.nranks; ++r) {
      const std::vector<fa_tile_desc> sub(g.t32.begin() + cut[r], g.t32.begin() + cut[r + 1]);
      std::vector<size_t> sc;
      cut_tiles(sub, nchunks, &sc, cut_align(g.elem));
      std::vector<int64_t>& b = p->clo[r];
      b.assign(nchunks + 1, p->lo[r + 1]);
      b[0] = p->lo[r];
      for (int c = 1; c < nchunks; ++c)
        if (sc[c] < sub.size()) b[c] = sub[sc[c]].start;
      if (r == g.rank)   // this rank's chunk c = tiles [cut_out[c], cut_out[c + 1])
        for (size_t c = 0; c <= (size_t)nchunks; ++c) cut_out->push_back(cut[r] + sc[c]);
    }
  } else if (p->mode == FA_MODE_CHAINED) {
    chain_geo(g, nchunks, &p->cg, vec_out, cut_out, tails_out, tidx_out);
    p->range = p->cg.range;
  } else {
    chain_geo(g, 1, &p->cg, vec_out, cut_out, tails_out, tidx_out);
    p->range = p->cg.range;
    return block_geo(g, *vec_out, &p->bg);
  }
  return FA_OK;
}

std::vector<fa_xfer> schedule(const RoundGeo& p, int root, bool weighted) {
  Sched S;
  if (p.mode == FA_MODE_SHARDED) sched_sharded(p.g, p.range, p.xchg, root, weighted, &S);
  else if (p.mode == FA_MODE_STRIPED) sched_striped(p.g, p.clo, root, weighted, &S);
  else if (p.mode == FA_MODE_CHAINED) sched_chained(p.g, p.cg, root, weighted, &S);
  else sched_blocked(p.g, p.cg, p.bg, root, &S);
  return S.ops;
}

// ---------------------------------------------------------- stream rules ---
bool on_comm_stream(const fa_xfer& x) {
  if (is_comm(x.op)) return true;
  switch (x.op) {
    case FA_X_K_SUM:
    case FA_X_K_ZERO:
    case FA_X_K_STACK:
    case FA_X_K_PART:                                // (the zero planes of PIN only)
    case FA_X_K_BLOCK:
    case FA_X_K_SCALE: return false;                 // read local inputs only
    case FA_X_K_STRIPE: return false;                // reads_exchanged: joined below
    case FA_X_K_CHAIN: return x.src == FA_B_STATE;   // after the state's hop
    default: return true;                            // read exchanged data
  }
}

// A compute-stream kernel that reads data exchanged in EARLIER steps (r06:
// the striped round's chunk reduce, beside the next chunk's exchange).  The
// executor records the communication stream's position at the start of the
// step — after the previous steps' groups, before this step's — and the
// caller's stream waits for it before the kernel, so the kernel overlaps
// this step's group.  A schedule must not give such a kernel data its own
// step's group writes (tests/schedsim.py checks it).
bool reads_exchanged(const fa_xfer& x) { return x.op == FA_X_K_STRIPE; }

// Buffers that kernels on the caller's (compute) stream write: partial sums,
// stacked raw columns, the blocked mode's outgoing partial and local block
// sums, and the state / result of a chain segment without a predecessor.
// An exchange or a comm-stream kernel that reads one of them waits for the
// compute stream first; the others (partials in transit, received planes,
// owners' block stripes, gathered rows, client buckets) need not, so they
// overlap the local kernels.  No exchange writes a buffer a compute-stream
// kernel reads or writes (received planes and stripes are comm-side only).
bool user_written(int b) {
  return b == FA_B_PARTIAL || b == FA_B_STACK || b == FA_B_TAILP || b == FA_B_BSUM ||
         b == FA_B_STATE || b == FA_B_OUT || b == FA_B_FIN || b == FA_B_STRIPE ||
         b == FA_B_WSTAGE;
}
bool needs_compute(const fa_xfer& x) { return user_written(x.src); }

// ============================================================ cost model ==
// (r06; fedagg_comm.h fa_round_model.)  Every
// rank's schedule replayed in virtual time under the executor's stream rules
// (fedcomm.hip execute): per rank the communication stream (tc) and the
// caller's stream (tu).  tests/roundmodel.py restates it and checks it
// against this.
// The model's constants: fedagg_comm.h's FA_MODEL_* unless the process
// environment sets a positive FA_MODEL_LINK_GBPS / FA_MODEL_HBM_GBPS /
// FA_MODEL_GROUP_US / FA_MODEL_KERNEL_US (read once), so numbers measured on
// a multi-GPU node re-rank the forms without a rebuild.
namespace {

struct ModelConst {
  double link_gbps, hbm_gbps, group_us, kernel_us;
};
double env_or(const char* name, double dflt, bool allow_zero) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const double x = std::strtod(v, &end);
  return (end && *end == '\0' && (x > 0.0 || (allow_zero && x == 0.0))) ? x : dflt;
}
const ModelConst& mc() {
  static const ModelConst c{env_or("FA_MODEL_LINK_GBPS", FA_MODEL_LINK_GBPS, false),
                            env_or("FA_MODEL_HBM_GBPS", FA_MODEL_HBM_GBPS, false),
                            env_or("FA_MODEL_GROUP_US", FA_MODEL_GROUP_US, true),
                            env_or("FA_MODEL_KERNEL_US", FA_MODEL_KERNEL_US, true)};
  return c;
}
inline double us_link(double bytes) { return bytes / (mc().link_gbps * 1e3); }
inline double us_hbm(double bytes) { return bytes / (mc().hbm_gbps * 1e3); }

int popc(unsigned v) { return __builtin_popcount(v); }

// HBM bytes a kernel op reads and writes (the columns it covers; count 0 =
// the vector columns, V elements); the scalar-column stacks and their
// reductions are a few KB and cost only their launch.
double kernel_bytes(const fa_xfer& x, int n_total, int64_t V, int es) {
  const double cols = (double)(x.count > 0 ? x.count : V);
  const double b = (double)es * cols;
  switch (x.op) {
    case FA_X_K_SUM:
    case FA_X_K_STRIPE:
    case FA_X_K_FOLD:
    case FA_X_K_PART:
    case FA_X_K_BLOCK: return (x.nrows + 1) * b;
    case FA_X_K_CONT: return (x.nrows + 2) * b;
    case FA_X_K_CHAIN: {
      const int lin = x.src == FA_B_STATE ? popc(fa_chain_levels(x.row0, n_total)) : 0;
      const int lout = x.dst == FA_B_STATE ? popc(fa_chain_levels(x.row0 + x.nrows, n_total)) : 1;
      // (the state planes are fp32 whatever the clients hold; a finishing
      // segment writes one row of the bucket's type)
      const int out = x.dst == FA_B_STATE ? 4 * std::max(lout, 1) : es;
      return (double)(x.nrows * es + 4 * lin + out) * cols;
    }
    case FA_X_K_COPY: return x.dst == FA_B_BLK ? 0.0 : 2 * b;
    case FA_X_K_DIV: return 2 * b;
    case FA_X_K_ZERO: return b;
    case FA_X_K_SCALE: return 2.0 * x.nrows * b;
    default: return 0.0;   // K_STACK, K_TAILS
  }
}

// (es: bytes per element of the floating bucket, 2 in a 16-bit round; the
// cascade's state planes and the gathered weights are fp32 in every round)
double elem_bytes(const fa_xfer& x, int es) {
  const int buf = x.op == FA_X_RECV ? x.dst : x.src;
  const int idx = x.op == FA_X_RECV ? x.dst_index : x.src_index;
  if (is_i64(buf, idx)) return 8.0;
  if (buf == FA_B_STATE || is_weights(buf, idx)) return 4.0;
  return (double)es;
}

// A collective's bytes on each link direction of a rank (ring algorithms).
double coll_link_bytes(const fa_xfer& x, int W, int esz) {
  const double es = elem_bytes(x, esz), n = (double)x.count * es;
  switch (x.op) {
    case FA_X_ALLGATHER:
      return x.src == FA_B_PARTIAL ? n * (W - 1) / W : n * (W - 1);
    case FA_X_BCAST: return n;
    case FA_X_ALLREDUCE: return 2.0 * n * (W - 1) / W;
    default: return n * (W - 1) / W;   // REDUCE, REDUCE_SCATTER, GATHER
  }
}

int model_schedules(const std::vector<std::vector<fa_xfer>>& sch, int n_total, int64_t V,
                    fa_round_cost* out, int es = 4) {
  const int W = (int)sch.size();
  std::vector<size_t> pos(W, 0);
  std::vector<char> posted(W, 0);
  std::vector<double> tc(W, 0.0), tu(W, 0.0), post(W, 0.0), ev3(W, 0.0);
  std::vector<double> hbm(W, 0.0);
  std::vector<std::vector<double>> lout(W, std::vector<double>(W, 0.0)),
      lin(W, std::vector<double>(W, 0.0));
  std::vector<int> groups(W, 0);
  // p2p matching: the post times of each channel's sends / receives in order
  std::map<std::pair<int, int>, std::vector<double>> sendt, recvt;
  std::map<uint64_t, std::vector<double>> collt;
  std::vector<uint64_t> cseq(W, 0);
  struct Pend {
    std::vector<std::pair<int, size_t>> p2p;  // (op index, channel position)
    std::vector<uint64_t> coll;
  };
  std::vector<Pend> pend(W);
  int steps = 0;
  for (;;) {
    bool progress = false, done = true;
    for (int r = 0; r < W; ++r) {
      const std::vector<fa_xfer>& o = sch[r];
      if (pos[r] >= o.size()) continue;
      done = false;
      const int step = o[pos[r]].step;
      size_t e = pos[r];
      while (e < o.size() && o[e].step == step) ++e;
      steps = std::max(steps, step + 1);
      if (!posted[r]) {
        ev3[r] = tc[r];
        bool join = false, comm = false;
        for (size_t i = pos[r]; i < e; ++i)
          if (is_comm(o[i].op)) {
            comm = true;
            join |= needs_compute(o[i]);
          }
        if (join) tc[r] = std::max(tc[r], tu[r]);
        post[r] = tc[r];
        pend[r] = Pend();
        for (size_t i = pos[r]; i < e; ++i) {
          const fa_xfer& x = o[i];
          if (x.op == FA_X_SEND) {
            auto& v = sendt[{r, x.peer}];
            pend[r].p2p.push_back({(int)i, v.size()});
            v.push_back(post[r]);
          } else if (x.op == FA_X_RECV) {
            auto& v = recvt[{x.peer, r}];
            pend[r].p2p.push_back({(int)i, v.size()});
            v.push_back(post[r]);
          } else if (is_comm(x.op)) {
            const uint64_t q = cseq[r]++;
            auto& v = collt[q];
            if (v.empty()) v.assign(W, -1.0);
            v[r] = post[r];
            pend[r].coll.push_back(q);
          }
        }
        if (comm) ++groups[r];
        posted[r] = 1;
        progress = true;
      }
      // complete once every peer has posted the matching operations
      double start = post[r];
      bool ok = true;
      for (const auto& pe : pend[r].p2p) {
        const fa_xfer& x = o[pe.first];
        const auto& v = x.op == FA_X_SEND ? recvt[{r, x.peer}] : sendt[{x.peer, r}];
        if (v.size() <= pe.second) {
          ok = false;
          break;
        }
        start = std::max(start, v[pe.second]);
      }
      for (uint64_t q : pend[r].coll) {
        if (!ok) break;
        for (double t : collt[q]) {
          if (t < 0) {
            ok = false;
            break;
          }
          start = std::max(start, t);
        }
      }
      if (!ok) continue;
      // the group
      std::vector<double> go(W, 0.0), gi(W, 0.0);
      double ghbm = 0.0, gcoll = 0.0;
      bool comm = false;
      for (size_t i = pos[r]; i < e; ++i) {
        const fa_xfer& x = o[i];
        if (!is_comm(x.op)) continue;
        comm = true;
        if (x.op == FA_X_SEND || x.op == FA_X_RECV) {
          const double b = (double)x.count * elem_bytes(x, es);
          (x.op == FA_X_SEND ? go : gi)[x.peer] += b;
          (x.op == FA_X_SEND ? lout : lin)[r][x.peer] += b;
          ghbm += b;
        } else {
          const double b = coll_link_bytes(x, W, es);
          gcoll += b;
          ghbm += 2.0 * b;
        }
      }
      if (comm) {
        double link = gcoll;
        for (int q = 0; q < W; ++q) link = std::max(link, std::max(go[q], gi[q]));
        tc[r] = start + mc().group_us + std::max(us_link(link), us_hbm(ghbm));
        hbm[r] += ghbm;
      }
      // the kernels
      for (size_t i = pos[r]; i < e; ++i) {
        const fa_xfer& x = o[i];
        if (is_comm(x.op)) continue;
        const double kb = kernel_bytes(x, n_total, V, es);
        const double dur = mc().kernel_us + us_hbm(kb);
        hbm[r] += kb;
        if (on_comm_stream(x)) {
          if (needs_compute(x)) tc[r] = std::max(tc[r], tu[r]);
          tc[r] += dur;
        } else {
          if (reads_exchanged(x)) tu[r] = std::max(tu[r], ev3[r]);
          tu[r] += dur;
        }
      }
      pos[r] = e;
      posted[r] = 0;
      progress = true;
    }
    if (done) break;
    if (!progress) return set_err(FA_E_INVAL, "fa_round_model: the schedules deadlock");
  }
  fa_round_cost c{};
  for (int r = 0; r < W; ++r) {
    c.model_us = std::max(c.model_us, std::max(tc[r], tu[r]));
    c.hbm_bytes_max = std::max(c.hbm_bytes_max, hbm[r]);
    for (int q = 0; q < W; ++q)
      c.link_bytes_max = std::max(c.link_bytes_max, std::max(lout[r][q], lin[r][q]));
    c.groups = std::max(c.groups, groups[r]);
  }
  c.steps = steps;
  *out = c;
  return FA_OK;
}

// One rank: every form is the plain reduction (fedcomm.hip make_round), one
// kernel reading n_total buckets and writing one.
fa_round_cost one_rank_cost(const Geo& g) {
  fa_round_cost c{};
  c.hbm_bytes_max =
      (double)(g.n_total + 1) *
      ((double)elem_size(g.elem) * (double)g.f32_numel + 8.0 * (double)g.i64_numel);
  c.model_us = mc().kernel_us + us_hbm(c.hbm_bytes_max);
  c.steps = 1;
  return c;
}

// Every rank's schedule of a form, from one geometry.
int all_schedules(const Geo& base, int mode, int nchunks, int xchg, int root, bool weighted,
                  std::vector<std::vector<fa_xfer>>* sch, int64_t* V) {
  sch->assign(base.nranks, {});
  *V = 0;
  for (const fa_tile_desc& t : base.t32)
    if (t.kind == 0) *V += t.count;
  for (int r = 0; r < base.nranks; ++r) {
    RoundGeo p;
    p.mode = mode;
    p.xchg = xchg;
    p.req_chunks = nchunks;
    p.g = base;
    p.g.rank = r;
    p.g.n_local = base.counts[r];
    p.g.lo_slot = base.first[r];
    std::vector<fa_tile_desc> vec, tails;
    std::vector<size_t> cut;
    std::vector<int64_t> tidx;
    const int rc = build_round(&p, nchunks, &vec, &cut, &tails, &tidx);
    if (rc) return rc;
    (*sch)[r] = schedule(p, root, weighted);
  }
  return FA_OK;
}

// The default entry's choice (fa_multi_select_layout): the exact form and
// chunk count with the lowest modelled time; ties keep the earlier candidate
// (blocked, then chained, then striped, fewer chunks first).
// A 16-bit bucket (base.elem): the striped form, and with `chain16` the
// chained one — the same chunk counts, the same order of candidates.
int select_form(const Geo& base, unsigned mflags, int* mode, int* nchunks, double* us,
                bool chain16 = false) {
  const bool h16 = base.elem != FA_ELEM_F32;
  if (h16 && (mflags & FA_MULTI_REASSOCIATE))
    return set_err(FA_E_INVAL, "fa_multi_select: the re-associated round runs on fp32 buckets");
  if (h16 && base.nranks == 1) {
    *mode = chain16 ? FA_MODE_CHAINED : FA_MODE_STRIPED;
    *nchunks = 1;
    if (us) *us = one_rank_cost(base).model_us;
    return FA_OK;
  }
  if (mflags & FA_MULTI_REASSOCIATE) {
    *mode = FA_MODE_SHARDED;
    *nchunks = 8;
    if (us) *us = -1.0;
    return FA_OK;
  }
  if (base.nranks == 1) {   // every form is the plain reduction
    *mode = first_wide_block(1, base.counts.data(), nullptr, nullptr) < 0 ? FA_MODE_BLOCKED
                                                                         : FA_MODE_CHAINED;
    *nchunks = 1;
    if (us) *us = one_rank_cost(base).model_us;
    return FA_OK;
  }
  int root = -1;
  if (!(mflags & FA_MULTI_ROOT_ALL))
    for (int r = 0; r < base.nranks; ++r)
      if (base.counts[r] > 0) root = r;
  struct Cand {
    int mode, nchunks;
  };
  std::vector<Cand> cand;
  if (!h16 && first_wide_block(base.nranks, base.counts.data(), nullptr, nullptr) < 0)
    cand.push_back({FA_MODE_BLOCKED, 1});
  if (!h16 || chain16)
    for (int c : {4, 8, 16, 32}) cand.push_back({FA_MODE_CHAINED, c});
  for (int c : {1, 2, 4, 8}) cand.push_back({FA_MODE_STRIPED, c});
  double best = 0.0;
  *mode = -1;
  for (const Cand& k : cand) {
    std::vector<std::vector<fa_xfer>> sch;
    int64_t V = 0;
    int rc = all_schedules(base, k.mode, k.nchunks, FA_XCHG_REDUCE, root, false, &sch, &V);
    if (rc) return rc;
    fa_round_cost c{};
    if ((rc = model_schedules(sch, base.n_total, V, &c, elem_size(base.elem)))) return rc;
    if (*mode < 0 || c.model_us < best) {
      best = c.model_us;
      *mode = k.mode;
      *nchunks = k.nchunks;
    }
  }
  if (us) *us = best;
  return FA_OK;
}

}  // namespace
}  // namespace fa_sched

// ====================================================== host-only view =====
using namespace fa_sched;

namespace {

// fa_describe_round[_elem]; `who`: the entry called, for the messages.
int describe_round(const char* who, int mode, int nranks, int rank, const int* counts,
                   const fa_seg* seg32, int nseg32, int64_t f32_numel, const fa_seg* seg64,
                   int nseg64, int64_t i64_numel, int nchunks, int exchange, unsigned flags,
                   int root, int weighted, fa_xfer* ops, int cap, int* nops, int elem,
                   unsigned ropts = 0) {
  if (!nops) return set_err(FA_E_INVAL, "%s: nops is NULL", who);
  *nops = 0;
  int rc = check_round_args(who, mode, &nchunks, exchange, root, nranks);
  if (rc) return rc;
  if ((rc = check_round_opts(who, elem, mode, weighted, ropts))) return rc;
  RoundGeo p;
  p.mode = mode;
  p.xchg = exchange;
  p.req_chunks = nchunks;
  rc = make_geo(nranks, rank, counts, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, flags,
                who, &p.g, elem);
  if (rc) return rc;
  std::vector<fa_tile_desc> vec, tails;
  std::vector<size_t> cut;
  std::vector<int64_t> tidx;
  if ((rc = build_round(&p, nchunks, &vec, &cut, &tails, &tidx))) return rc;
  const std::vector<fa_xfer> s = schedule(p, root, weighted != 0);
  *nops = (int)s.size();
  if (ops) {
    if (cap < (int)s.size())
      return set_err(FA_E_RANGE, "%s: %d ops, capacity %d", who, (int)s.size(), cap);
    std::copy(s.begin(), s.end(), ops);
  }
  return FA_OK;
}

// fa_round_model[_elem]
int round_model(const char* who, int mode, int nranks, const int* counts, const fa_seg* seg32,
                int nseg32, int64_t f32_numel, const fa_seg* seg64, int nseg64,
                int64_t i64_numel, int nchunks, int exchange, unsigned flags, int root,
                int weighted, fa_round_cost* out, int elem, unsigned ropts = 0) {
  if (!out) return set_err(FA_E_INVAL, "%s: out is NULL", who);
  int rc = check_round_args(who, mode, &nchunks, exchange, root, nranks);
  if (rc) return rc;
  if ((rc = check_round_opts(who, elem, mode, weighted, ropts))) return rc;
  Geo g;
  rc = make_geo(nranks, 0, counts, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, flags, who,
                &g, elem);
  if (rc) return rc;
  if (nranks == 1) {
    *out = one_rank_cost(g);
    return FA_OK;
  }
  std::vector<std::vector<fa_xfer>> sch;
  int64_t V = 0;
  if ((rc = all_schedules(g, mode, nchunks, exchange, root, weighted != 0, &sch, &V))) return rc;
  return model_schedules(sch, g.n_total, V, out, elem_size(g.elem));
}

}  // namespace

extern "C" {

int fa_describe_round(int mode, int nranks, int rank, const int* counts, const fa_seg* seg32,
                      int nseg32, int64_t f32_numel, const fa_seg* seg64, int nseg64,
                      int64_t i64_numel, int nchunks, int exchange, unsigned flags, int root,
                      int weighted, fa_xfer* ops, int cap, int* nops) {
  return describe_round("fa_describe_round", mode, nranks, rank, counts, seg32, nseg32, f32_numel,
                        seg64, nseg64, i64_numel, nchunks, exchange, flags, root, weighted, ops,
                        cap, nops, FA_ELEM_F32);
}

// (FA_ELEM_F32 is the fp32 entry exactly, its name in the messages included)
int fa_describe_round_elem(int mode, int nranks, int rank, const int* counts,
                           const fa_seg* seg32, int nseg32, int64_t f32_numel,
                           const fa_seg* seg64, int nseg64, int64_t i64_numel, int nchunks,
                           int exchange, unsigned flags, int root, int weighted, fa_xfer* ops,
                           int cap, int* nops, int elem) {
  return describe_round(elem == FA_ELEM_F32 ? "fa_describe_round" : "fa_describe_round_elem",
                        mode, nranks, rank, counts, seg32, nseg32, f32_numel, seg64, nseg64,
                        i64_numel, nchunks, exchange, flags, root, weighted, ops, cap, nops, elem);
}

// (no option bit: the _elem entry exactly, its name in the messages included)
int fa_describe_round_opts(int mode, int nranks, int rank, const int* counts, const fa_seg* seg32,
                           int nseg32, int64_t f32_numel, const fa_seg* seg64, int nseg64,
                           int64_t i64_numel, int nchunks, int exchange, unsigned flags, int root,
                           int weighted, fa_xfer* ops, int cap, int* nops, int elem,
                           unsigned ropts) {
  if (!ropts)
    return fa_describe_round_elem(mode, nranks, rank, counts, seg32, nseg32, f32_numel, seg64,
                                  nseg64, i64_numel, nchunks, exchange, flags, root, weighted, ops,
                                  cap, nops, elem);
  return describe_round("fa_describe_round_opts", mode, nranks, rank, counts, seg32, nseg32,
                        f32_numel, seg64, nseg64, i64_numel, nchunks, exchange, flags, root,
                        weighted, ops, cap, nops, elem, ropts);
}

int fa_model_constants(double* link_gbps, double* hbm_gbps, double* group_us,
                       double* kernel_us) {
  const ModelConst& c = mc();
  if (link_gbps) *link_gbps = c.link_gbps;
  if (hbm_gbps) *hbm_gbps = c.hbm_gbps;
  if (group_us) *group_us = c.group_us;
  if (kernel_us) *kernel_us = c.kernel_us;
  return FA_OK;
}

int fa_round_model(int mode, int nranks, const int* counts, const fa_seg* seg32, int nseg32,
                   int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
                   int nchunks, int exchange, unsigned flags, int root, int weighted,
                   fa_round_cost* out) {
  return round_model("fa_round_model", mode, nranks, counts, seg32, nseg32, f32_numel, seg64,
                     nseg64, i64_numel, nchunks, exchange, flags, root, weighted, out, FA_ELEM_F32);
}

int fa_round_model_elem(int mode, int nranks, const int* counts, const fa_seg* seg32, int nseg32,
                        int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
                        int nchunks, int exchange, unsigned flags, int root, int weighted,
                        fa_round_cost* out, int elem) {
  return round_model(elem == FA_ELEM_F32 ? "fa_round_model" : "fa_round_model_elem", mode, nranks,
                     counts, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel, nchunks, exchange,
                     flags, root, weighted, out, elem);
}

int fa_round_model_opts(int mode, int nranks, const int* counts, const fa_seg* seg32, int nseg32,
                        int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
                        int nchunks, int exchange, unsigned flags, int root, int weighted,
                        fa_round_cost* out, int elem, unsigned ropts) {
  if (!ropts)
    return fa_round_model_elem(mode, nranks, counts, seg32, nseg32, f32_numel, seg64, nseg64,
                               i64_numel, nchunks, exchange, flags, root, weighted, out, elem);
  return round_model("fa_round_model_opts", mode, nranks, counts, seg32, nseg32, f32_numel, seg64,
                     nseg64, i64_numel, nchunks, exchange, flags, root, weighted, out, elem, ropts);
}

// The default multi-GPU entry's choice (fedcomm.hip fa_multi_plan_create):
// select_form; e1 only on request (FA_MULTI_REASSOCIATE).
int fa_multi_select_layout(int nranks, const int* counts, const fa_seg* seg32, int nseg32,
                           int64_t f32_numel, const fa_seg* seg64, int nseg64, int64_t i64_numel,
                           unsigned flags, unsigned mflags, int* mode, int* nchunks,
                           double* model_us) {
  if (!mode || !nchunks) return set_err(FA_E_INVAL, "fa_multi_select: mode/nchunks is NULL");
  *mode = -1;
  *nchunks = 0;
  if (nranks < 1 || !counts) return set_err(FA_E_INVAL, "fa_multi_select: bad arguments");
  if (mflags & ~(unsigned)(FA_MULTI_REASSOCIATE | FA_MULTI_ROOT_ALL))
    return set_err(FA_E_INVAL, "fa_multi_select: unknown flags 0x%x", mflags);
  Geo g;
  const int rc = make_geo(nranks, 0, counts, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                          flags, "fa_multi_select", &g);
  if (rc) return rc;
  return select_form(g, mflags, mode, nchunks, model_us);
}

// ... on a bucket of `elem` elements.  FA_ELEM_F32 without an option: the
// fp32 entry exactly.  16-bit: the striped form, or with FA_ROUND_CHAIN16 the
// better of striped and chained.
int fa_multi_select_layout_elem(int nranks, const int* counts, const fa_seg* seg32, int nseg32,
                                int64_t f32_numel, const fa_seg* seg64, int nseg64,
                                int64_t i64_numel, unsigned flags, unsigned mflags, int elem,
                                unsigned ropts, int* mode, int* nchunks, double* model_us) {
  if (elem == FA_ELEM_F32 && !ropts)
    return fa_multi_select_layout(nranks, counts, seg32, nseg32, f32_numel, seg64, nseg64,
                                  i64_numel, flags, mflags, mode, nchunks, model_us);
  const char* who = "fa_multi_select_layout_elem";
  if (!mode || !nchunks) return set_err(FA_E_INVAL, "%s: mode/nchunks is NULL", who);
  *mode = -1;
  *nchunks = 0;
  if (nranks < 1 || !counts) return set_err(FA_E_INVAL, "%s: bad arguments", who);
  if (mflags & ~(unsigned)(FA_MULTI_REASSOCIATE | FA_MULTI_ROOT_ALL))
    return set_err(FA_E_INVAL, "%s: unknown flags 0x%x", who, mflags);
  if (ropts & ~(unsigned)FA_ROUND_CHAIN16)
    return set_err(FA_E_INVAL, "%s: unknown round options 0x%x", who, ropts);
  if (elem == FA_ELEM_F32)
    return set_err(FA_E_INVAL, "%s: FA_ROUND_CHAIN16 names the chained round on an fp16 / bf16 "
                               "bucket (an fp32 bucket chains without it)", who);
  Geo g;
  const int rc = make_geo(nranks, 0, counts, seg32, nseg32, f32_numel, seg64, nseg64, i64_numel,
                          flags, who, &g, elem);
  if (rc) return rc;
  return select_form(g, mflags, mode, nchunks, model_us, (ropts & FA_ROUND_CHAIN16) != 0);
}

int fa_multi_select(int nranks, const int* counts, unsigned mflags, int* mode) {
  if (!mode) return set_err(FA_E_INVAL, "fa_multi_select: mode is NULL");
  // the nominal layout: one fp32 tensor of 2^24 elements
  const fa_seg seg{0, (int64_t)1 << 24};
  int nchunks = 0;
  return fa_multi_select_layout(nranks, counts, &seg, 1, seg.numel, nullptr, 0, 0,
                                FA_PLAN_GAPS_ARE_PADDING, mflags, mode, &nchunks, nullptr);
}

}  // extern "C"
