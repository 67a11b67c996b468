#!/usr/bin/env python
"""In-process FedAvg simulator: N clients on ONE device, one process, same data split and
round semantics as bench.py / the client agents -- for engine-vs-engine parity runs.

Every client is a full :class:`LocalTrainer` (own model, momentum, data shard); a round
is: each client trains one local epoch on its shard -> the uniform mean of every
float state entry and the floor mean of the int64 BN counters (reference
src/server.py:155-179, fedmi.parallel.fedavg semantics) is loaded into every client
-> the global model is evaluated on the full test set.  ``--engine native`` uses
the fedmi HIP engines (bf16 activations, fp32 master), ``--engine fp32`` plain
PyTorch fp32 (FEDMI_TORCH_PATH=1), both from the same initial weights.

  python tools/fedavg_sim.py --model resnet18 --clients 2 --noniid 2 --rounds 8 --engine fp32
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

N_TRAIN, N_TEST, BATCH = 50000, 10000, 128
ATTACKS = ("none", "signflip", "scale", "nan")


def attack_state(kind: str, start: torch.Tensor, x: torch.Tensor, scale: float) -> torch.Tensor:
    """What a simulated Byzantine client sends instead of its trained state ``x``, given the round's starting model:
    ``signflip``: start - A (x - start); ``scale``: start + A (x - start); ``nan``: all NaN."""
    if kind == "signflip":
        return start - scale * (x - start)
    if kind == "scale":
        return start + scale * (x - start)
    if kind == "nan":
        return torch.full_like(x, float("nan"))
    raise ValueError(f"attack must be one of {ATTACKS[1:]}, not {kind!r}")


def robust_stack(robust, states, nat=None):
    """The robust aggregate of the simulated clients' float states (a list of equal-length fp32 tensors) and the cut
    counts: ``robust_reduce`` (csrc/kernels/robust.hip) on a GPU, its torch twin elsewhere."""
    from fedmi import native
    from fedmi.parallel.robust import robust_reduce_torch

    W, n = len(states), states[0].numel()
    b = robust.cfg.b_eff(W)
    if not states[0].is_cuda:
        return robust_reduce_torch(torch.stack(states), b)
    nat = nat or native.require()
    dev = states[0].device
    ld = (n + 3) & ~3
    rows = torch.zeros((W, ld), dtype=torch.float32, device=dev)
    for r, x in enumerate(states):
        rows[r, :n].copy_(x)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    partial = torch.zeros((max(1, nat.robust_partials(n)), 16), dtype=torch.int64, device=dev)
    stats = torch.zeros(16, dtype=torch.int64, device=dev)
    nat.robust_reduce(native.stream_handle(dev), rows.data_ptr(), ld, W, n, b, out.data_ptr(), partial.data_ptr(),
                      stats.data_ptr())
    return out, stats[:W]


def _eval_batch_bn(tr) -> None:
    """Diagnostic (PyTorch engines): evaluate the global model with batch-statistics BN instead of the averaged
    running statistics (train-mode BN at momentum 0, so the running buffers are left as they are)."""
    from torch.nn.modules.batchnorm import _BatchNorm

    m = tr.model
    bns = [b for b in m.modules() if isinstance(b, _BatchNorm)]
    mom = [b.momentum for b in bns]
    for b in bns:
        b.momentum = 0.0
    orig_eval = m.eval
    m.eval = lambda: m.train()
    try:
        with torch.no_grad():
            tr.evaluate()
    finally:
        m.eval = orig_eval
        for b, v in zip(bns, mom):
            b.momentum = v
        m.eval()


def _run_seed(a, seed, data, dev, out) -> None:
    from fedmi.engine import build_trainer
    from fedmi.engine.base import TrainerConfig
    from fedmi.engine.data import contiguous_schedule, label_shard_indices, strided_schedule
    from fedmi.parallel.client_opt import make_client_opt
    from fedmi.parallel.dp import make_dp
    from fedmi.parallel.robust import make_robust
    from fedmi.parallel.server_opt import make_server_opt

    cfg = TrainerConfig(seed=seed, lr=a.lr, augment=not a.no_augment, use_graph=not a.no_graph)
    W = a.clients
    clients = []
    init = None
    for r in range(W):
        tr = build_trainer(a.model, data, dev, cfg, init_state=init)
        if a.engine == "bf16":
            def run(x, m=tr.model):
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    return m(x).float()
            tr._run = run
        if init is None:        # one shared init (rank-0 broadcast, reference quirk A7 fixed)
            init = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
        if a.noniid > 0:
            shards = label_shard_indices(data.train.y.cpu().numpy(), W, a.noniid, seed=0)
            tr.set_train_data(data.train.subset(shards[r]))
            tr.set_schedule(*contiguous_schedule(len(shards[r]), BATCH))
        else:
            tr.set_schedule(*strided_schedule(a.n_train, BATCH, r, W))
        clients.append(tr)
    # one server optimizer for the simulated federation: it steps the stacked mean (held in client 0's state)
    # before the result is copied into every client; parameter / buffer split from n_params()
    server = make_server_opt(a.server_opt, clients[0], a.server_lr, a.server_beta1, a.server_beta2, a.server_tau)
    # one client optimizer per simulated client (its own c_i / anchor); the mean of their delta stands in for
    # the second all-reduce
    copts = [make_client_opt(a.client_opt, tr, a.client_mu) for tr in clients]
    # one DP guard per simulated client: its own key, anchor and draw counter; each adds its 1/sqrt(W) noise share
    dps = [make_dp(a.dp_clip, tr, a.dp_noise, a.dp_delta, a.dp_seed, who=f"seed{seed}/client{r}")
           for r, tr in enumerate(clients)]
    robust = make_robust(a.robust, clients[0], a.robust_trim)
    for rnd in range(1, a.rounds + 1):
        t0 = time.perf_counter()
        tstats = []
        start = clients[0].float_state().clone() if a.attack != "none" else None   # every client holds it
        for tr in clients:
            tr.train_epoch()
            tstats.append(tr.train_stats())
        with torch.no_grad():
            dmean = None
            if copts[0] is not None:
                for co in copts:
                    co.finish_round()
                if copts[0].delta is not None:
                    dmean = torch.stack([co.delta for co in copts]).mean(0)
            for tr, dp in zip(clients, dps):
                if dp is not None:
                    dp.privatize(tr, W)
            for tr in clients[W - a.attackers:] if a.attack != "none" else ():
                tr.float_state().copy_(attack_state(a.attack, start, tr.float_state(), a.attack_scale))
            cut = None
            if robust is not None and W > 1:
                mean, cut = robust_stack(robust, [tr.float_state() for tr in clients])
            else:
                mean = torch.stack([tr.float_state() for tr in clients]).mean(0)
            ints = [torch.div(sum(bs), W, rounding_mode="floor")
                    for bs in zip(*[[b.clone() for b in tr.int_state()] for tr in clients])]
            if server is not None:
                clients[0].float_state().copy_(mean)
                server.step(clients[0])
                mean = clients[0].float_state().clone()
            for tr in clients:
                tr.float_state().copy_(mean)
                for b, v in zip(tr.int_state(), ints):
                    b.copy_(v)
                tr.after_aggregate()
            for tr, co in zip(clients, copts):
                if co is not None:
                    co.begin_round(tr, dmean)
            for tr, dp in zip(clients, dps):
                if dp is not None:
                    dp.begin_round(tr)
        if a.bn_eval == "batch":
            _eval_batch_bn(clients[0])
        else:
            clients[0].evaluate()
        ev = clients[0].eval_stats()
        torch.cuda.synchronize() if dev.type == "cuda" else None
        rec = {"round": rnd, "engine": a.engine, "model": a.model, "clients": W, "lr": a.lr, "seed": seed,
               "data": a.data, "server_opt": a.server_opt,
               "server_lr": server.cfg.lr if server is not None else None,
               "client_opt": a.client_opt, "client_mu": a.client_mu if a.client_opt == "fedprox" else None,
               "deterministic": bool(a.deterministic),
               "augment": not a.no_augment, "graph": not a.no_graph,
               "split": f"noniid-{a.noniid}" if a.noniid else "strided-iid", "bn_eval": a.bn_eval,
               "train_loss": [round(s.loss, 4) for s in tstats], "train_acc": [round(s.acc, 2) for s in tstats],
               "test_loss": round(ev.loss, 4), "test_acc": round(ev.acc, 2),
               "finite": bool(torch.isfinite(mean).all()), "round_s": round(time.perf_counter() - t0, 3)}
        if dps[0] is not None:
            # the eval above synchronised, so every client's stats row of this round is on the host
            rows = [dp.round_stats() for dp in dps]
            rec.update(dp_clip=a.dp_clip, dp_noise=a.dp_noise, dp_delta=a.dp_delta, dp_epsilon=rows[0]["dp_epsilon"],
                       dp_norm=[round(r.get("dp_norm", -1.0), 4) for r in rows],
                       dp_scale=[round(r.get("dp_scale", -1.0), 4) for r in rows])
        if robust is not None:
            rec.update(robust_kind=a.robust, robust_trim=robust.cfg.b_eff(W),
                       robust_cut=cut.tolist() if cut is not None else None)
        if a.attack != "none":
            rec.update(attack=a.attack, attackers=a.attackers, attack_scale=a.attack_scale)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--clients", type=int, default=2)
    ap.add_argument("--noniid", type=int, default=0, help="label shards per client (0 = strided IID)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--engine", choices=["native", "fp32", "bf16"], default="native",
                    help="bf16: PyTorch autocast bf16 (torch's own mixed precision of the same model)")
    ap.add_argument("--data", default="synthetic-cifar10",
                    help="dataset spec (fedmi.engine.data.make_dataset): synthetic-cifar10 | synthetic-cifar10-easy | ...")
    ap.add_argument("--n-train", type=int, default=N_TRAIN)
    ap.add_argument("--n-test", type=int, default=N_TEST)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--seeds", default="", help="comma list: run each seed in turn (one process)")
    ap.add_argument("--out", default=None, help="JSONL, one record per round")
    ap.add_argument("--no-augment", action="store_true", help="no crop/flip (diagnostics)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of graph replay (diagnostics)")
    ap.add_argument("--deterministic", action="store_true",
                    help="PyTorch engines: deterministic algorithms (MIOpen / rocBLAS deterministic kernels), so two "
                         "runs of the fp32 reference agree and a parity gap is the engine's, not reference noise")
    ap.add_argument("--bn-eval", choices=["running", "batch"], default="running",
                    help="batch: evaluate the global model with batch-statistics BN (diagnostic, PyTorch engines)")
    from fedmi.parallel.server_opt import add_server_opt_flags

    add_server_opt_flags(ap)
    from fedmi.parallel.client_opt import add_client_opt_flags

    add_client_opt_flags(ap)
    from fedmi.parallel.dp import add_dp_flags, check_dp_flags

    add_dp_flags(ap)
    from fedmi.parallel.robust import add_robust_flags, check_robust_flags

    add_robust_flags(ap)
    ap.add_argument("--attack", default="none", choices=list(ATTACKS),
                    help="simulated Byzantine clients (the simulator only): the last --attackers clients send "
                         "start - A (x - start) (signflip), start + A (x - start) (scale) or all NaN (nan) instead of "
                         "their trained state x")
    ap.add_argument("--attackers", type=int, default=1, metavar="K")
    ap.add_argument("--attack-scale", type=float, default=10.0, metavar="A")
    a = ap.parse_args(argv)
    if a.client_mu < 0:
        ap.error("--client-mu must be >= 0")
    check_dp_flags(a, ap.error)
    check_robust_flags(a, ap.error)
    if a.attack != "none" and not 1 <= a.attackers <= a.clients:
        ap.error("--attackers must lie in 1..--clients")
    if a.bn_eval == "batch" and a.engine == "native":
        ap.error("--bn-eval batch needs a PyTorch engine (fp32 / bf16)")
    if a.engine in ("fp32", "bf16"):
        os.environ["FEDMI_TORCH_PATH"] = "1"
    if a.deterministic:
        from fedmi.utils.stats import make_deterministic

        make_deterministic()

    from fedmi.engine.data import make_dataset

    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    data = make_dataset(a.data, device=dev, n_train=a.n_train, n_test=a.n_test, seed=0)
    seeds = [int(v) for v in a.seeds.split(",")] if a.seeds else [a.seed]
    out = open(a.out, "w") if a.out else None
    for seed in seeds:
        _run_seed(a, seed, data, dev, out)
        torch.cuda.empty_cache() if dev.type == "cuda" else None
    return 0


if __name__ == "__main__":
    sys.exit(main())
