"""Shared by the tests of the chained multi-GPU round on fp16 / bf16 buckets
(test_chain16_cpu.py, test_gpu_dist_chain16.py): the schedule replay with
16-bit client, result and stack buffers and fp32 state planes, the weighted
expectation, and the oracle arithmetic backend of dist.ChainAggregator.

Layouts, client data and the unweighted expectation are tests/round16.py's."""
import numpy as np
import torch

import round16 as R
import schedsim
from oracle import torch_order as O
from test_dist_gloo import OracleChainBackend

F32 = np.float32


def expected16w(lay, dtype, bits, weights, i64=None):
    """round16.expected16 for a weighted round: per segment
    narrow(O.weighted_sum0(widen(bits), w)); the int64 keys stay means."""
    exp, inside, e64 = R.expected16(lay, dtype, bits, i64)
    w = np.asarray(weights, F32)
    with np.errstate(all="ignore"):
        for o, m in lay.segs32:
            o, m = int(o), int(m)
            exp[o:o + m] = R.narrow(O.weighted_sum0(R.widen(bits[:, o:o + m], dtype), w), dtype)
    return exp, inside, e64


class SimChain16(schedsim.Sim):
    """tests/schedsim.py on the 16-bit chained round: CLIENT, OUT, FIN and the
    stacked / gathered scalar columns (STACK / GATHER index 0) hold uint16
    patterns, the STATE planes fp32; STACK / GATHER index 2 hold the ranks'
    fp32 weights.  The chain kernel widens, multiplies by the local weight and
    continues the cascade state; the finishing one divides (unless weighted)
    and rounds once.  The scalar columns travel raw and are multiplied by the
    gathered weights where they are reduced."""

    def __init__(self, layout, dtype, tiles, counts, clients16, clients64, weights=None):
        super().__init__(layout, tiles, counts, clients16, clients64, weights)
        self.dtype = dtype
        n16 = layout.f32_numel
        for b in self.buf:
            b["OUT"] = np.full(n16, R.FILL16, np.uint16)
            b["FIN"] = np.full(n16, R.FILL16, np.uint16)
            b["STACK"][0] = np.full(self.nmax * self.trow, R.FILL16, np.uint16)
            b["GATHER"][0] = np.full(self.W * self.nmax * self.trow, R.FILL16, np.uint16)
            b["STACK"].append(np.full(self.nmax, np.nan, F32))
            b["GATHER"].append(np.full(self.W * self.nmax, np.nan, F32))

    def _wide(self, s, st, cnt):
        v = R.widen(self.c32[s][st:st + cnt], self.dtype)
        return v if self.w is None else (v * self.w[s]).astype(F32)

    def _kernel(self, r, x):
        op, b = x["op"], self.buf[r]
        n_loc = self.counts[r]
        slots = range(self.first[r], self.first[r] + n_loc)
        if op == "K_STACK":
            T = len(self.tidx)
            for j, s in enumerate(slots):
                if T:
                    b["STACK"][0][j * self.trow:j * self.trow + T] = self.c32[s][self.tidx]
                if self.layout.i64_numel:
                    w64 = self.layout.i64_numel
                    b["STACK"][1][j * w64:(j + 1) * w64] = self.c64[s]
            if self.w is not None:
                b["STACK"][2][:] = 0
                b["STACK"][2][:n_loc] = self.w[self.first[r]:self.first[r] + n_loc]
        elif op == "K_CHAIN":
            row0, nr = x["row0"], x["nrows"]
            lin = O.chain_levels(row0, self.n)
            lout = O.chain_levels(row0 + nr, self.n)
            with np.errstate(all="ignore"):
                for st, cnt, _ in self._tiles_in(x["offset"], x["count"], vec_only=True):
                    acc = None
                    if x["src"] == "STATE":
                        acc = [b["STATE"][l][st:st + cnt].copy() if lin & (1 << l)
                               else np.zeros(cnt, F32) for l in range(4)]
                    elif lin:
                        raise AssertionError(f"rank {r}: chain kernel at row {row0} without state")
                    acc = O.cascade_state([self._wide(s, st, cnt) for s in range(row0, row0 + nr)],
                                          row0, self.n, acc)
                    if x["dst"] == "STATE":
                        for l in range(4):
                            if lout & (1 << l):
                                b["STATE"][l][st:st + cnt] = acc[l]
                    else:
                        s = O.cascade_finish(acc)
                        res = s if self.w is not None else (s / F32(self.n)).astype(F32)
                        b[x["dst"]][st:st + cnt] = R.narrow(res, self.dtype)
        elif op == "K_TAILS":
            rows = [(rr, j) for rr in range(self.W) for j in range(self.counts[rr])]
            if len(self.tidx):
                assert self.t32_gathered, "K_TAILS before the scalar columns' gather"
                g = b["GATHER"][0]
                comp = {int(e): k for k, e in enumerate(self.tidx)}
                with np.errstate(all="ignore"):
                    for st, cnt, kind in self.tail:
                        ks = [comp[int(e)] for e in range(st, st + cnt)]
                        data = []
                        for rr, j in rows:
                            v = R.widen(g[(rr * self.nmax + j) * self.trow:][ks], self.dtype)
                            if self.w is not None:      # the gathered weight, not self.w
                                v = (v * b["GATHER"][2][rr * self.nmax + j]).astype(F32)
                            data.append(v)
                        res = (F32(0) + schedsim._column_sum(kind, data)).astype(F32)
                        if self.w is None:
                            res = (res / F32(self.n)).astype(F32)
                        b["OUT"][st:st + cnt] = R.narrow(res, self.dtype)
            gathered, self.t32_gathered = self.t32_gathered, False
            super()._kernel(r, x)                       # the int64 keys
            self.t32_gathered = gathered
        else:
            raise AssertionError(f"{op} in a 16-bit chained round")


class OracleChainBackend16(OracleChainBackend):
    """dist.ChainAggregator's backend on CPU tensors of a 16-bit dtype: the
    chained kernels restated with the oracle on the widened values, fp32 state
    planes, one rounding at the finish; the scalar columns reduced over raw
    16-bit rows with every row's weight."""

    def __init__(self, layout, dtype, chunks, compact):
        super().__init__(layout, chunks, compact)
        self.dtype = dtype

    def _wide(self, t, w):
        v = R.widen(R.bits_of(t), self.dtype)
        return v if w is None else (v * F32(w)).astype(F32)

    def chain(self, c, clients32, row0, n_total, state, state_in, out, plane, weights=None):
        assert state.dtype == torch.float32
        lev_in = O.chain_levels(row0, n_total)
        lev_out = O.chain_levels(row0 + len(clients32), n_total)
        with np.errstate(all="ignore"):
            for st, cnt, _ in self.chunks[c][2]:
                st, cnt = int(st), int(cnt)
                rows = [self._wide(t[st:st + cnt], None if weights is None else weights[j])
                        for j, t in enumerate(clients32)]
                acc = None
                if state_in:
                    acc = [state[l * plane + st:l * plane + st + cnt].numpy().copy()
                           if lev_in & (1 << l) else np.zeros(cnt, F32) for l in range(4)]
                acc = O.cascade_state(rows, row0, n_total, acc)
                if out is None:
                    for l in range(4):
                        if lev_out & (1 << l):
                            state[l * plane + st:l * plane + st + cnt] = torch.from_numpy(acc[l])
                else:
                    s = O.cascade_finish(acc)
                    if weights is None:
                        s = (s / F32(n_total)).astype(F32)
                    out[st:st + cnt] = R.as_tensor(R.narrow(s, self.dtype), self.dtype)

    def tails(self, rows32, tidx, out32, weighted, weights=None):
        assert weighted == (weights is not None), "16-bit rows travel raw: weights, or a mean"
        n = len(rows32)
        with np.errstate(all="ignore"):
            for cs, cnt, kind in self.compact:
                cs, cnt = int(cs), int(cnt)
                data = [self._wide(r[cs:cs + cnt], None if weights is None else weights[k])
                        for k, r in enumerate(rows32)]
                res = (F32(0) + schedsim._column_sum(kind, data)).astype(F32)
                if not weighted:
                    res = (res / F32(n)).astype(F32)
                out32[tidx[cs:cs + cnt]] = R.as_tensor(R.narrow(res, self.dtype), self.dtype)
