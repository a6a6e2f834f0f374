"""The long-launch layout of test_client_loop_instances_on_a_long_launch
(tests/test_gpu_parity.py), shared: a launch of three and more rounds of
resident workgroups, whose full tiles take the client loop (pipe_rule), with
adversarial client data generated on the device and the windows the oracle
checks."""
import numpy as np
import torch

from feddct_amd.layout import BucketLayout

BIG = 6   # index of the long key


def long_launch_case(lib, n, weighted, dev, seed=0):
    """(layout, plan, x [n, F] on the device, windows [(offset, numel)]).
    The windows are the small keys whole and the long key's head, middle and
    end (its last partial tile and ILP-4 tail columns); each is a whole-tensor
    oracle call over columns of the same class."""
    probe = lib.Plan(np.array([[0, 4096]], np.int64), 4096)
    slots = probe.launch_shape(n, weighted)[1]
    assert slots > 0
    big = 3 * slots * 2048 + 2050 + 13
    sizes = [100, 4096, 7, 3000, 1, 64, big, 3, 9000]
    man = {"keys": [{"key": f"k{j}", "shape": [m], "dtype": "float32"}
                    for j, m in enumerate(sizes)]}
    layout = BucketLayout.from_manifest(man)
    plan = lib.Plan(layout.segs32, layout.f32_numel, flags=lib.FA_PLAN_GAPS_ARE_PADDING)
    F = max(layout.f32_numel, 64)
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + n + seed)
    x = torch.rand((n, F), generator=g, device=dev) * 2 - 1
    ex = torch.randint(-20, 21, (n, F), generator=g, device=dev).to(torch.float32)
    x = (x * torch.pow(2.0, ex)).contiguous()
    del ex
    return layout, plan, x, windows(layout)


def big_key(layout):
    o, m = layout.segs32[BIG]
    return int(o), int(m)


def head_window(layout):
    return big_key(layout)[0], 8192


def end_window(layout):
    o_big, m_big = big_key(layout)
    t = m_big % 32
    return o_big + m_big - 64 - t - 4096, 4096 + 64 + t


def windows(layout):
    o_big, m_big = big_key(layout)
    w = [(int(o), int(m)) for j, (o, m) in enumerate(layout.segs32) if j != BIG]
    return w + [head_window(layout), (o_big + (m_big // 2) // 64 * 64, 8192), end_window(layout)]
