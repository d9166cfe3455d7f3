"""Measurements of profiles/nme_eval.md (needs a GPU): (a) ops.nme_topk
device time against the torch fp32 composition normalize -> matmul -> topk,
the two alternating in one process, device events, 3 warm-up launches each;
(b) the NME step (build_prototypes + evaluate_nme) against evaluate() over
the same validation set inside one engine run, each timed on its second
invocation with a host clock around a device synchronize. Prints one JSON
line per measurement.

    python tools/nmebench.py
"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cilfw import ops  # noqa: E402

dev = "cuda:0"
res = {}


def ev_time(fn, rounds):
    ts = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(True), torch.cuda.Event(True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def part_a(N, C, D, rounds):
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.relu(torch.randn(N, D, device=dev, generator=g))
    ex = torch.relu(torch.randn(C * 4, D, device=dev, generator=g))
    protos = ops.nme_prototypes(ex, list(range(0, 4 * C + 1, 4)))
    tg = torch.randint(0, C, (N,), device=dev, generator=g)

    def ours():
        return ops.nme_topk(x, protos, 5, tg)

    def comp():
        xh = torch.nn.functional.normalize(x, dim=1, eps=1e-12)
        return torch.topk(xh @ protos.T, 5, dim=1)

    for _ in range(3):
        ours(), comp()
    torch.cuda.synchronize()
    to, tc = [], []
    for _ in range(rounds):  # alternate the two
        to += ev_time(ours, 1)
        tc += ev_time(comp, 1)
    i1 = ours()[0].long()
    i2 = comp()[1]
    to.sort(), tc.sort()
    flop = 2.0 * N * C * D
    res[f"a_{N}x{C}x{D}"] = dict(
        ours_ms_median=to[len(to) // 2], ours_ms_min=to[0],
        comp_ms_median=tc[len(tc) // 2], comp_ms_min=tc[0],
        ours_tflops_median=flop / to[len(to) // 2] / 1e9,
        comp_tflops_median=flop / tc[len(tc) // 2] / 1e9,
        top1_agree=(i1[:, 0] == i2[:, 0]).float().mean().item(),
        rounds=rounds)
    print(json.dumps(res[f"a_{N}x{C}x{D}"]), flush=True)


def part_b():
    import cilfw.engine as E
    import cilfw.cil.nme as M
    from cilfw.config import parse_args
    t = {}
    o_eval, o_build, o_nme = E.evaluate, M.build_prototypes, M.evaluate_nme

    def timed(name, fn):
        def w(*a, **k):
            fn(*a, **k)  # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            t.setdefault(name, []).append(time.perf_counter() - t0)
            return r
        return w

    E.evaluate = timed("evaluate", o_eval)
    M.build_prototypes = timed("build_prototypes", o_build)
    M.evaluate_nme = timed("evaluate_nme", o_nme)
    args = parse_args([
        # no CIFAR pickle at this path: the CIFAR-100-shaped synthetic set
        "--data_set", "cifar100", "--data_path", "/nonexistent",
        "--backbone", "resnet18", "--num_bases", "100", "--increment", "10",
        "--num_epochs", "1", "--batch_size", "128", "--workers", "0",
        "--memory_size", "2000", "--eval_every_epoch", "0", "--no_aug",
        "--aa", "", "--color_jitter", "0", "--seed", "0", "--gpu_data",
        "--nme_eval"])
    E.run(args)
    res["b"] = dict(t, ratio=(t["build_prototypes"][-1]
                              + t["evaluate_nme"][-1]) / t["evaluate"][-1])
    print(json.dumps(res["b"]), flush=True)


part_a(10000, 100, 512, 30)
part_a(50000, 1000, 2048, 12)
part_b()
