"""Generate tests/golden/h16_goldens.npz by running the REFERENCE's own
``server_aggregate`` (train_fedavg.py:138-149) on fp16 and bf16 modules, on
the CPU.  Build container only (the reference is imported by make_golden.py's
recipe); run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_h16_golden.py

Nothing from the reference is copied: the fixture holds the PRNG inputs and
the reference's outputs, 16-bit values as int16 bit patterns.

Outputs
  tests/golden/h16_manifest.json   keys / shapes (dtype "h16": the case's 16-bit type)
  tests/golden/h16_goldens.npz     <dtype>/n<N>/in<i>/<key>, <dtype>/n<N>/out/<key>
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import Holder, import_reference  # noqa: E402

NS = [3, 17, 33]
SHAPES = [[], [7], [3, 3], [33], [100], [2049]]
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def h16_manifest():
    keys = [{"key": f"t{j}", "shape": s, "dtype": "h16"} for j, s in enumerate(SHAPES)]
    keys.append({"key": "num_batches_tracked", "shape": [], "dtype": "int64"})
    return {"name": "h16", "keys": keys, "ns": NS}


def holder(man, tdt):
    m = Holder({"keys": [dict(e, dtype="float32" if e["dtype"] == "h16" else e["dtype"])
                         for e in man["keys"]]})
    return m.to(tdt)   # floating parameters only; the int64 buffers stay


def fill(m, client, n):
    g = torch.Generator().manual_seed(1000 + client)
    base = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if v.dtype == torch.int64:
                v.copy_(torch.randint(0, 1 << 30, v.shape, generator=g))
                continue
            b = torch.randn(v.shape, generator=base) * 0.05
            x = b * (1 + 0.01 * torch.randn(v.shape, generator=g))
            if v.numel() >= 33:   # a stretch of values whose mean is a 16-bit subnormal
                flat = x.reshape(-1)
                tiny = torch.finfo(v.dtype).tiny
                flat[8:24] = tiny * torch.rand(16, generator=g) * (2.0 if client % 2 else 0.0)
            v.copy_(x)


def main():
    ref = import_reference()
    torch.set_num_threads(1)
    man = h16_manifest()
    gold = {}
    for name, tdt in DTYPES.items():
        for n in NS:
            g = holder(man, tdt)
            clients = [holder(man, tdt) for _ in range(n)]
            for i, c in enumerate(clients):
                fill(c, i, n)
                for k, v in c.state_dict().items():
                    gold[f"{name}/n{n}/in{i}/{k}"] = (
                        v.numpy().copy() if v.dtype == torch.int64
                        else v.detach().view(torch.int16).numpy().copy())
            ref["fedavg"].server_aggregate(g, clients)
            for k, v in g.state_dict().items():
                assert v.dtype == (torch.int64 if k == "num_batches_tracked" else tdt)
                gold[f"{name}/n{n}/out/{k}"] = (
                    v.numpy().copy() if v.dtype == torch.int64
                    else v.detach().view(torch.int16).numpy().copy())
            for c in clients:
                for k, v in c.state_dict().items():
                    assert torch.equal(v, g.state_dict()[k]), "broadcast"
    path = os.path.join(HERE, "h16_goldens.npz")
    np.savez_compressed(path, **gold)
    with open(os.path.join(HERE, "h16_manifest.json"), "w") as f:
        json.dump(man, f, indent=0)
    print(len(gold), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
