"""Generate tests/golden/mixed16_goldens.npz by running the REFERENCE's own
``server_aggregate`` (train_fedavg.py:138-149) with an fp32 global model over
fp16 / bf16 clients, on the CPU.  Build container only (the reference is
imported by make_golden.py's recipe); run from the repository root:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_mixed16_golden.py

The inputs are the ones already stored in h16_goldens.npz (the clients of
make_h16_golden.py); nothing from the reference is copied.  Only outputs are
written: the fp32 global the reference leaves, as int32 bit patterns.  The
clients it leaves must equal h16_goldens.npz's ``out`` arrays (the pure
16-bit round gives the clients the same bits); that is asserted here, so the
test reads the clients' expected bits from that fixture.

Outputs
  tests/golden/mixed16_goldens.npz   <dtype>/n<N>/global/<key>
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
from make_h16_golden import DTYPES, holder  # noqa: E402


def main():
    ref = import_reference()
    torch.set_num_threads(1)
    with open(os.path.join(HERE, "h16_manifest.json")) as f:
        man = json.load(f)
    src = np.load(os.path.join(HERE, "h16_goldens.npz"))
    gold = {}
    for name, tdt in DTYPES.items():
        for n in man["ns"]:
            g = Holder({"keys": [dict(e, dtype="float32" if e["dtype"] == "h16" else e["dtype"])
                                 for e in man["keys"]]})
            clients = [holder(man, tdt) for _ in range(n)]
            with torch.no_grad():
                for i, c in enumerate(clients):
                    for k, v in c.state_dict().items():
                        t = torch.from_numpy(src[f"{name}/n{n}/in{i}/{k}"].copy())
                        v.copy_(t if v.dtype == torch.int64 else t.view(tdt))
            ref["fedavg"].server_aggregate(g, clients)
            for k, v in g.state_dict().items():
                assert v.dtype == (torch.int64 if k == "num_batches_tracked" else torch.float32)
                gold[f"{name}/n{n}/global/{k}"] = (
                    v.numpy().copy() if v.dtype == torch.int64
                    else v.detach().view(torch.int32).numpy().copy())
            for c in clients:
                for k, v in c.state_dict().items():
                    want = src[f"{name}/n{n}/out/{k}"]
                    got = v if v.dtype == torch.int64 else v.detach().view(torch.int16)
                    assert v.dtype == (torch.int64 if k == "num_batches_tracked" else tdt)
                    assert np.array_equal(got.numpy(), want), (name, n, k, "clients differ from "
                                                               "the pure 16-bit round's")
    path = os.path.join(HERE, "mixed16_goldens.npz")
    np.savez_compressed(path, **gold)
    print(len(gold), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
