"""The data-parallel step as the driver's multi-GPU bench runs it (config 3: DDP over RCCL,
the reference's ``utils/distributed.py:415-428`` around ``main.py:331-386``), on the one-GPU box:

* ``bench.py --gpus 2 --full`` end to end: the launcher starts two ranks (gloo: RCCL refuses two ranks on one
  device), each runs the eager DP step with the bucketed all-reduce; one JSON line, ``n_gpus`` and
  ``ranks_seen`` 2, a finite loss and bitwise identical parameters on both ranks after the last step;
* the all-reduce buckets of every weight-gradient schedule the DP backward can take (the default
  cuts of the grouped launch at each full round of tiles, ``RP_WGRAD_GROUP_LAYERS`` cuts, per-layer
  split-K, fp32)
  tile ``[0, trainable_numel)`` exactly once, in reverse layout order;
* the captured DP step (``CapturedTrainStep(capture_collectives=True)``: RCCL all-reduces captured into
  the HIP graph, tile cut active, backward writing the gradients) on a one-rank RCCL group gives bitwise
  the parameters and Adam moments of eager DP steps, with and without the per-bucket Adam
  (``FusedAdam.overlap_with``: each bucket updated right after its wait), which is also bitwise the
  whole-buffer update in eager DP steps, here and on two gloo ranks;
* the DP update pinned to the oracle: two ranks through ``MultiGPUStrategy.setup`` / ``wrap_model`` /
  the HIP backward / ``FusedAdam`` against the CPU oracle's gradients of each rank's batch, averaged,
  then ``torch.optim.Adam`` (the reference's ``main.py:331-369``, ``utils/distributed.py:415-428``).

Every process group here is created with a bounded timeout (60 s), so a stuck rendezvous or collective
raises with a stack instead of stalling the suite, and the parent notices a worker that died without
answering within two seconds (``_wait``).
"""
import datetime
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _heartbeat(request, msg):
    """A progress line on the terminal, past pytest's capture: a long multi-process test is not then
    taken for a hang by a runner that watches the output."""
    capman = request.config.pluginmanager.getplugin("capturemanager")
    if capman is None:  # capture disabled (-p no:capture): plain print reaches the terminal
        print(f"\n[{msg}]", flush=True)
        return
    with capman.global_and_fixture_disabled():
        print(f"\n[{msg}]", flush=True)


def _wait(q, p, request, name, limit, trace=None):
    """The worker's (status, result): polled every 2 s, a progress line every 20 s; ("timeout", log tail)
    when it has not answered within ``limit`` seconds, ("died", exit code + log tail) as soon as it
    has exited without answering (a crashed worker must not look like a hang)."""
    import queue
    import time
    t0 = last_beat = time.time()

    def log_tail():
        if trace and os.path.exists(trace):
            with open(trace) as f:
                return f.read()[-6000:]
        return ""

    try:
        while True:
            try:
                return q.get(timeout=2)
            except queue.Empty:
                now = time.time()
                if not p.is_alive():
                    try:  # an answer put just before exiting
                        return q.get(timeout=1)
                    except queue.Empty:
                        return "died", f"{name}: exited with code {p.exitcode} without answering\n{log_tail()}"
                if now - t0 > limit:
                    return "timeout", log_tail() or f"{name}: no answer after {now - t0:.0f}s"
                if now - last_beat >= 20:
                    last_beat = now
                    tail = log_tail().strip().splitlines()
                    _heartbeat(request, f"{name} {now - t0:.0f}s: {tail[-1] if tail else 'running'}")
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.kill()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(420)
def test_bench_two_ranks_gloo(dev, request, tmp_path):
    import time
    env = dict(os.environ, RP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    out, err = tmp_path / "bench.out", tmp_path / "bench.err"
    with open(out, "w") as fo, open(err, "w") as fe:
        proc = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3",
                                 "--warmup", "1", "--full"], stdout=fo, stderr=fe, text=True, env=env, cwd=ROOT)
        t0 = time.time()
        while True:
            try:
                proc.wait(timeout=20)
                break
            except subprocess.TimeoutExpired:
                if time.time() - t0 > 400:
                    proc.kill()
                    proc.wait()
                    break
                _heartbeat(request, f"bench.py --gpus 2 (gloo) {time.time() - t0:.0f}s")
    stdout, stderr = out.read_text(), err.read_text()
    assert proc.returncode == 0, stderr[-4000:]
    lines = [l for l in stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, stdout
    res = json.loads(lines[0])
    print({k: res[k] for k in ("value", "ms_per_step", "n_gpus", "ranks_seen", "param_checksums", "execution")})
    assert res["n_gpus"] == 2 and res["ranks_seen"] == 2
    assert res["config"]["parallelism"] == "dp2" and res["comm"]["backend"] == "gloo"
    c = res["comm"]  # where the DP step's time goes (the driver's SCALE lines)
    assert c["adam"] == "per bucket after its wait" and c["buckets_per_step"] >= 2
    assert c["exposed_ms"] is not None and c["exposed_ms"] >= 0 and c["max_bucket_wait_ms"] >= 0
    assert len(c["wgrad_launch_ms"]) >= 3 and all(t > 0 for t in c["wgrad_launch_ms"])
    assert res["execution"].startswith("eager")
    assert torch.isfinite(torch.tensor(res["loss"])).item()
    assert res["value"] > 0 and len(res["rank_ms_per_step"]) == 2
    cs = res["param_checksums"]
    assert len(cs) == 2 and cs[0] == cs[1], cs


def _tiling_worker(port, q, cases):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    try:
        import torch.distributed as dist
        from repurpose_amd.distributed import GradAllReducer
        from repurpose_amd.MMCTransformer import MMCTransformer
        from tests.test_model_gpu import TRI, make_batch, to_dev
        dist.init_process_group("gloo", rank=0, world_size=1, timeout=datetime.timedelta(seconds=60))
        dev = torch.device("cuda", 0)
        b = to_dev(make_batch(TRI, 2, 128, [128, 90], seed=3), dev)
        out = []
        for name, dtype, env in cases:
            saved = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                torch.manual_seed(1)
                m = MMCTransformer(**dict(TRI, self_num_layers=16), compute_dtype=dtype).to(dev).train()
                m.DROPOUT = 0.0
                red = GradAllReducer(m, bucket_mb=4.0)
                (m.losses(*m(b))["cls_loss"] / 2).backward()
                launched = list(red.launched)
                red.wait()
                torch.cuda.synchronize()
                out.append((name, m.trainable_numel(), launched))
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        q.put(("ok", out))
    except Exception:
        import traceback
        q.put(("err", traceback.format_exc()))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_buckets_tile_the_gradient_buffer(dev, request):
    cases = [("tile cut (default)", "bf16", {}),
             ("8-layer groups", "bf16", {"RP_WGRAD_GROUP_LAYERS": "8"}),
             ("4-layer groups", "bf16", {"RP_WGRAD_GROUP_LAYERS": "4"}),
             ("one 16-layer group", "bf16", {"RP_WGRAD_GROUP_LAYERS": "16"}),
             ("per-layer split-K", "bf16", {"RP_WGRAD_GROUPED": "0"}),
             ("fp32", "fp32", {})]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_tiling_worker, args=(_port(), q, cases))
    p.start()
    status, res = _wait(q, p, request, "bucket tiling worker", 240)
    assert status == "ok", res
    for name, n, launched in res:
        assert launched, name
        # reverse layout order: each bucket ends where the previous one began
        assert launched[0][1] == n, (name, launched[0], n)
        for a, c in zip(launched, launched[1:]):
            assert c[1] == a[0], (name, a, c)
        assert launched[-1][0] == 0, (name, launched[-1])
        assert sum(hi - lo for lo, hi in launched) == n, name  # exactly once
        print(f"{name}: {len(launched)} buckets")


def _captured_worker(q, trace):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import faulthandler
    import time
    tf = open(trace, "w", buffering=1)
    t0 = time.time()

    def mark(stage):  # stage log (stacks on stderr every 30 s) for a run that does not finish
        tf.write(f"{time.time() - t0:7.1f}s {stage}\n")
        sys.stderr.write(f"[captured worker] {time.time() - t0:7.1f}s {stage}\n")
        sys.stderr.flush()

    faulthandler.dump_traceback_later(30, repeat=True, file=sys.stderr)
    try:
        import torch.distributed as dist
        from repurpose_amd.distributed import GradAllReducer
        from repurpose_amd.graph import CapturedTrainStep
        from repurpose_amd.MMCTransformer import MMCTransformer
        from repurpose_amd.optim import FusedAdam
        from tests.test_model_gpu import TRI, make_batch, to_dev
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        mark("init_process_group")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=60))
        mark("process group up")
        cfg = dict(TRI, self_num_layers=16)
        batches = [{k: v for k, v in to_dev(make_batch(cfg, 2, 128, [128, 100], seed=40 + i), dev).items()
                    if torch.is_tensor(v)} for i in range(4)]

        def fresh():
            torch.manual_seed(5)
            m = MMCTransformer(**cfg, compute_dtype="bf16").to(dev).train()
            m.DROPOUT = 0.0
            return m, FusedAdam(m, lr=1e-3, weight_decay=1e-4), GradAllReducer(m)

        me, oe, re_ = fresh()
        for i, b in enumerate(batches):
            oe.zero_grad()
            (me.losses(*me(b))["cls_loss"] / 2).backward()
            re_.wait()
            oe.step()
            torch.cuda.synchronize()
            mark(f"eager DP step {i}")
        n = me.trainable_numel()
        ok = []
        for overlap in [c == "1" for c in os.environ.get("RP_TEST_CAPTURE_CASES", "01")]:
            mg, og, rg = fresh()
            if overlap:  # set, but a captured step keeps the whole-buffer Adam (FusedAdam.overlap_with)
                og.overlap_with(rg)
            run = CapturedTrainStep(mg, og, {k: v.clone() for k, v in batches[0].items()}, warmup=1,
                                    capture_collectives=True)
            torch.cuda.synchronize()
            mark(f"captured (adam overlap {overlap})")
            for i, b in enumerate(batches):
                run.load(b)
                run.step()
                torch.cuda.synchronize()
                mark(f"replay {i}")
            ok.append((run._graph is not None, len(rg.launched) > 0,
                       torch.equal(mg.flat_params()[:n], me.flat_params()[:n]),
                       torch.equal(og._m, oe._m), torch.equal(og._v, oe._v)))
            # the graph (and the RCCL plan resources it holds) goes before the communicator it was
            # captured on is destroyed
            del run
            torch.cuda.synchronize()
            mark("graph released")
        # eager DP with the per-bucket Adam: bitwise the whole-buffer update
        mo, oo, ro = fresh()
        oo.overlap_with(ro)
        for i, b in enumerate(batches):
            oo.zero_grad()
            (mo.losses(*mo(b))["cls_loss"] / 2).backward()
            ro.wait()
            oo.step()
        torch.cuda.synchronize()
        ok.append((True, ro.on_bucket is not None, torch.equal(mo.flat_params()[:n], me.flat_params()[:n]),
                   torch.equal(oo._m, oe._m), torch.equal(oo._v, oe._v)))
        mark("eager overlap")
        q.put(("ok", ok))
    except Exception:
        import traceback
        q.put(("err", traceback.format_exc()))
    finally:
        faulthandler.cancel_dump_traceback_later()
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()
        mark("done")


@pytest.mark.timeout(300)
def test_captured_rccl_dp_step_equals_eager_dp(dev, tmp_path, request):
    trace = str(tmp_path / "captured_worker.log")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_captured_worker, args=(q, trace))
    p.start()
    status, res = _wait(q, p, request, "captured DP worker", 240, trace)
    assert status == "ok", res
    for name, (captured, hooked, params, m1, m2) in zip(("captured", "captured + per-bucket Adam",
                                                          "eager per-bucket Adam"), res):
        assert captured, f"{name}: the DP step was not captured"
        assert hooked, f"{name}: the backward issued no all-reduce"
        assert params and m1 and m2, (name, res)


# ------------------------------------------------------------------- DP update pinned to the oracle
DP_CFG = dict(vis_dim=512, aud_dim=2048, text_dim=384, d_model=512, self_num_layers=2, text_num_layers=3,
              cross_num_layers=3, num_heads=8)
DP_STEPS, DP_B, DP_T = 2, 2, 128
DP_LR, DP_WD = 1e-3, 1e-4


def _dp_batch(rank, step):
    """Rank ``rank``'s batch of step ``step``: B = 2 ragged sequences (its own data, as a
    DistributedSampler hands each rank)."""
    from tests.test_model_gpu import make_batch
    lens = [[DP_T, 77], [101, DP_T]][rank]
    b = make_batch(DP_CFG, DP_B, DP_T, lens, seed=1000 + 10 * rank + step)
    return {k: v for k, v in b.items() if torch.is_tensor(v)}


def _dp_oracle_worker(rank, world, port, q, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        from repurpose_amd.distributed import DistributedModel, MultiGPUStrategy
        from repurpose_amd.MMCTransformer import MMCTransformer
        from repurpose_amd.optim import FusedAdam
        s = MultiGPUStrategy(strategy="auto", backend="gloo", timeout=60)
        assert s.strategy == "ddp" and s.world_size == world and s.setup() is True
        torch.manual_seed(100 + rank)  # a different init per rank: wrap_model broadcasts rank 0's
        m = MMCTransformer(**DP_CFG, compute_dtype="fp32")
        m.DROPOUT = 0.0  # dropout off: the oracle runs in eval mode
        w = s.wrap_model(m)
        assert isinstance(w, DistributedModel)
        opt = FusedAdam(w.parameters(), lr=DP_LR, weight_decay=DP_WD)
        w.train()
        rec = {}
        for step in range(DP_STEPS):
            b = {k: v.to(s.device) for k, v in _dp_batch(rank, step).items()}
            opt.zero_grad()
            out = w(b)
            loss = w.module.losses(*out)["cls_loss"] / DP_B  # main.py:331: cls_loss / batch_size
            loss.backward()  # DDP: the HIP backward's hooks all-reduce the flat gradient (AVG)
            opt.step()
            torch.cuda.synchronize()
            rec[f"grad{step}"] = m.flat_grads()[:m.trainable_numel()].cpu().clone()
            rec[f"params{step}"] = m.flat_params().cpu().clone()
        torch.save(rec, os.path.join(outdir, f"rank{rank}.pt"))
        s.barrier()
        q.put((rank, "ok"))
    except Exception:
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_update_matches_oracle_adam(dev, tmp_path):
    """The data-parallel update against the reference computation done by the CPU oracle: two gloo ranks
    (sharing the box's GPU) each run their own ragged batch through ``MultiGPUStrategy.setup`` ->
    ``wrap_model`` (rank 0's parameters broadcast) -> the HIP fp32 forward / backward with the bucketed
    all-reduce -> ``FusedAdam``, two steps; the oracle (``oracle/mmct_oracle.py``, rank 0's init, eval
    mode = dropout off) computes each rank's ``cls_loss / B`` gradient, averages the two (DDP) and applies
    ``torch.optim.Adam(lr=1e-3, weight_decay=1e-4)``.  Checks, per step and parameter tensor:
    (a) the DP-averaged gradient within the fp32 gradient gate of
    ``test_model_gpu.py::test_backward_fp32_parity`` (2e-3 of the tensor's largest element) of the
    oracle's average; (b) the update: ``torch.optim.Adam`` replayed on the CPU with the HIP gradients
    gives the HIP parameters to 1e-6 of each tensor's largest parameter; (c) the whole chain: the
    parameters within 1e-5 of the oracle's (||difference|| / ||parameters||) on every element whose
    oracle gradient was at least 1e-2 of its tensor's largest at every step so far — Adam normalises
    each element's step, so an element with a tiny gradient moves by ~lr whatever its value and its
    fp32 rounding differences are amplified to O(lr) (there: at most 2 lr per step); for the
    zero-initialised tensors (biases, LayerNorm beta: their values ARE the updates) the updates within
    1e-4; reg_head untouched
    (no loss reaches it: torch skips ``grad is None``); both ranks bitwise equal."""
    from oracle.mmct_oracle import MMCTransformer as Oracle
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_dp_oracle_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = []
        for _ in procs:
            try:
                res.append(q.get(timeout=240))
            except Exception:
                res.append((-1, "no answer within 240 s: " + ", ".join(f"rank {i} exit {p.exitcode}"
                                                                       for i, p in enumerate(procs))))
                break
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    bad = [f"rank {rank}: {msg}" for rank, msg in sorted(res) if msg != "ok"]
    assert not bad, "\n".join(bad)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    for k in r0:
        assert torch.equal(r0[k], r1[k]), f"ranks differ in {k}"

    torch.manual_seed(100)
    ref = Oracle(**DP_CFG).eval()
    torch.manual_seed(100)
    replay = Oracle(**DP_CFG)  # torch Adam fed the HIP gradients: the update alone
    opt = torch.optim.Adam(ref.parameters(), lr=DP_LR, weight_decay=DP_WD)
    opt_r = torch.optim.Adam(replay.parameters(), lr=DP_LR, weight_decay=DP_WD)
    names = [n for n, _ in ref.named_parameters()]
    params, rparams = dict(ref.named_parameters()), dict(replay.named_parameters())
    sizes = [p.numel() for p in ref.parameters()]
    from repurpose_amd.MMCTransformer import MMCTransformer
    torch.manual_seed(100)
    layout = MMCTransformer(**DP_CFG, compute_dtype="fp32")
    base = layout.flat_params().data_ptr()
    offs = [(p.data_ptr() - base) // 4 for p in layout.parameters()]  # flat layout (views, 8-aligned)
    assert [n for n, _ in layout.named_parameters()] == names
    init = {n: p.detach().clone() for n, p in ref.named_parameters()}
    determined = {n: torch.ones_like(p, dtype=torch.bool) for n, p in ref.named_parameters()}
    worst_g = worst_u = worst_p = worst_z = 0.0
    for step in range(DP_STEPS):
        acc = None
        for rank in range(2):
            ref.zero_grad(set_to_none=True)
            b = _dp_batch(rank, step)
            (ref.losses(*ref(b))["cls_loss"] / DP_B).backward()
            g = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in ref.named_parameters()}
            acc = g if acc is None else {n: (None if v is None else v + g[n]) for n, v in acc.items()}
        g_hip, p_hip = r0[f"grad{step}"], r0[f"params{step}"]
        for n, off, size in zip(names, offs, sizes):
            p_ = params[n]
            p_.grad = None if acc[n] is None else acc[n] / 2  # DDP: the mean over ranks
            rparams[n].grad = None if acc[n] is None else g_hip[off:off + size].view_as(p_).clone()
            if acc[n] is not None:
                geff = p_.grad.abs()
                determined[n] &= geff >= 1e-2 * geff.max()
        opt.step()
        opt_r.step()
        for n, off, size in zip(names, offs, sizes):
            p_ref = params[n].detach()
            got_p = p_hip[off:off + size].view_as(p_ref)
            if n.startswith("reg_head."):
                assert torch.equal(got_p, init[n]), f"{n} moved (no loss reaches it: torch skips grad None)"
                continue
            gr = params[n].grad
            gscale = gr.abs().max().item() + 1e-12
            rel_g = (rparams[n].grad - gr).abs().max().item() / gscale
            worst_g = max(worst_g, rel_g)
            assert rel_g < 2e-3, f"step {step} {n}: averaged gradient rel err {rel_g:.2e}"
            pscale = p_ref.abs().max().item() + 1e-12
            rel_u = (got_p - rparams[n].detach()).abs().max().item() / pscale
            worst_u = max(worst_u, rel_u)
            assert rel_u < 1e-6, f"step {step} {n}: FusedAdam vs torch Adam on the same gradients: {rel_u:.2e}"
            d = (got_p - p_ref).abs()
            det = determined[n]
            # norm-relative over the determined elements.  Zero-initialised tensors (biases, LayerNorm beta)
            # hold nothing but the Adam updates after two steps (~lr each), so for them the figure is taken
            # relative to the update and bounded at 1e-4: Adam divides each element's step by its own
            # gradient's magnitude, so the fp32 gradient agreement (~1e-6 of the tensor's largest, check a)
            # becomes ~1e-4 of the step on an element 1e-2 of the largest
            zero_init = bool((init[n] == 0).all())
            ref_mag = (p_ref - init[n])[det].norm() if zero_init else p_ref[det].norm()
            rel_p = (d[det].norm() / (ref_mag + 1e-30)).item() if det.any() else 0.0
            if zero_init:
                worst_z = max(worst_z, rel_p)
                assert rel_p < 1e-4, f"step {step} {n}: zero-init parameters vs oracle, update rel err {rel_p:.2e}"
            else:
                worst_p = max(worst_p, rel_p)
                assert rel_p < 1e-5, f"step {step} {n}: parameters vs oracle + torch Adam rel err {rel_p:.2e}"
            assert (d <= 2 * DP_LR * (step + 1) * 1.001).all(), f"step {step} {n}: a parameter moved too far"
    print(f"worst averaged-gradient rel err {worst_g:.2e}, update (FusedAdam vs torch Adam) {worst_u:.2e}, "
          f"parameters vs oracle (determined elements) {worst_p:.2e}, zero-init tensors' updates {worst_z:.2e}")


def _overlap_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    try:
        import torch.distributed as dist
        from repurpose_amd.distributed import GradAllReducer
        from repurpose_amd.MMCTransformer import MMCTransformer
        from repurpose_amd.optim import FusedAdam
        from tests.test_model_gpu import TRI, make_batch, to_dev
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        dev = torch.device("cuda", 0)
        cfg = dict(TRI, self_num_layers=16)
        res = []
        for overlap in (False, True):
            torch.manual_seed(7)
            m = MMCTransformer(**cfg, compute_dtype="bf16").to(dev).train()
            m.DROPOUT = 0.0
            o = FusedAdam(m, lr=1e-3, weight_decay=1e-4)
            r = GradAllReducer(m, bucket_mb=4.0)
            if overlap:
                o.overlap_with(r)
            for step in range(2):
                b = to_dev(make_batch(cfg, 2, 128, [128, 70 + 30 * rank], seed=50 + 10 * rank + step), dev)
                o.zero_grad()
                (m.losses(*m(b))["cls_loss"] / 2).backward()
                r.wait()
                o.step()
            torch.cuda.synchronize()
            n = m.trainable_numel()
            res.append((m.flat_params()[:n].cpu(), o._m.cpu(), o._v.cpu(), m.lowp_weights()[:n].cpu()))
        q.put(("ok", tuple(bool(torch.equal(a, b)) for a, b in zip(*res))))
    except Exception:
        import traceback
        q.put(("err", traceback.format_exc()))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_per_bucket_adam_bitwise_two_gloo_ranks(dev, request):
    """FusedAdam.overlap_with on two gloo ranks (16 layers, 4 MB buckets: many per step): parameters, Adam
    moments and the bf16 operand copy after two steps are bitwise those of the whole-buffer update."""
    ctx = mp.get_context("spawn")
    port = _port()
    qs = [ctx.Queue() for _ in range(2)]
    ps = [ctx.Process(target=_overlap_worker, args=(r, 2, port, qs[r])) for r in range(2)]
    for p in ps:
        p.start()
    for r in range(2):
        status, res = _wait(qs[r], ps[r], request, f"per-bucket Adam rank {r}", 240)
        assert status == "ok", res
        assert all(res), (r, res)
