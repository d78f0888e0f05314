"""Step driver of cut_model: the discriminator half enqueued on a second stream under the generator's backward, and both halves replayed from
hipGraphs.  The model (cut_model.py) keeps what mirrors the reference -- forward, losses, networks -- and owns one `CUTStepDriver`, which keeps
the streams, the captured graphs and their guards.  `gate` is the one spelling of "option with environment override"."""
import os
import warnings
from dataclasses import dataclass

import torch

import joligen_amd
from .. import ops, parallel

# round 6: the history-pool draws of the early-D drivers run on the discriminator stream (JG_POOL_SIDE=0: on the main stream, as in round 5)
POOL_ON_SIDE = os.environ.get("JG_POOL_SIDE", "1") != "0"


def gate(opt, option, env, default=True, force=False):
    """An A/B switch: option `option` (absent: `default`) under the environment variable `env`, read at call time.  `env=0` switches the path
    off; `env=1` switches it on over a false option only with `force` (the tri-state gates JG_FORK_GAN / JG_GRAPH_G / JG_GRAPH_D;
    JG_EARLY_D / JG_NCE_REUSE_FEATS / JG_BATCHED_NCE switch off only)."""
    want = os.environ.get(env, "")
    return bool((getattr(opt, option, default) or (force and want == "1")) and want != "0")


class CapturedHalf:
    """The bookkeeping of one half of the step replayed from hipGraphs, without the device work (which the half hands in): the gate, at most
    three captured states (one per operand shape: a last, smaller batch of an epoch), the snapshot / restore of the state a canary touches,
    the canary's comparison, and the sticky fall-back to the eager half with its warning and `step_driver_note`."""

    def __init__(self, model, option, env, label, dropped, dbg, unsafe_note=None):
        self.model, self.option, self.env, self.label, self.dropped, self.dbg, self.unsafe_note = model, option, env, label, dropped, dbg, unsafe_note
        self.cache, self.failed = {}, False

    def ready(self):
        """option / environment, then the guards both halves share (a failed capture has left its reason in `step_driver_note`)"""
        m = self.model
        if not gate(m.opt, self.option, self.env, force=True):
            return False
        if not joligen_amd.HIP_GRAPHS_SAFE:
            m.step_driver_note = self.unsafe_note or m.step_driver_note      # (said by the discriminator half only)
            return False
        return not (self.failed or m.act_dtype == torch.float16 or m.niter <= 2 or ops.KERNEL_TIMING is not None)

    def get(self, key, nets, capture):
        """The captured state for operands `key` of the networks `nets`, or None (the eager half runs).  First use: `capture(restore)` captures,
        runs its canary and returns the state; whatever it raises drops this half for good.  `restore()` puts back what a replay touches --
        gradient arenas, spectral-norm vectors, BatchNorm statistics -- and runs once more after the capture, passed or failed."""
        key += (tuple(n.arena.p.data_ptr() for n in nets), tuple(n.training for n in nets))
        st = self.cache.get(key)
        if st is not None or self.failed or len(self.cache) >= 3:
            return st
        state = [n.arena.g for n in nets] + [b for n in nets for b in n.buffers()]
        saved = [t.clone() for t in state]

        def restore():
            for t, t0 in zip(state, saved):
                t.data.copy_(t0)      # .data: no version bump (frozen-BN tables key on versions; tensors saved by G's forward stay valid)

        try:
            st = self.cache[key] = capture(restore)
        except Exception as e:
            m = self.model
            ops.zero_pool_reset(m.device)
            warnings.warn(f"{self.option}: the {self.label} half stays eager ({e})")
            m.step_driver_note = (m.step_driver_note + "; " if m.step_driver_note else "") + f"{self.dropped}: {e}"
            self.failed = True
        restore()
        return st

    def check(self, first, second, tol, what, hint=""):
        """the canary: two replays from the same state, with eager launches in between, must agree"""
        if os.environ.get("JG_DBG_GRAPH_CANARY_FAIL") == self.dbg:      # tests: the fall-back path of a failing canary
            second = second * 1.5 + 1.0
        red = (lambda t: t.all()) if first.dim() else (lambda t: t)
        if not bool((red(torch.isfinite(first)) & red(torch.isfinite(second)) & red((first - second).abs() <= tol * first.abs() + 1e-6)).item()):
            raise RuntimeError(f"replays of {what} disagree after interleaved eager launches ({first.tolist()} vs {second.tolist()}){hint}")


@dataclass
class GenGraphs:
    """generator half: graph F (forward + losses) on static inputs, graph B (backward) in F's memory pool; `outs`: attribute -> tensor of F"""
    real_A: torch.Tensor
    real_B: torch.Tensor
    fwd: object = None
    bwd: object = None
    outs: dict = None
    ctx_A: torch.Tensor = None      # data_online_context_pixels: static copies of real_A_with_context / real_B_with_context
    ctx_B: torch.Tensor = None


@dataclass
class DiscGraph:
    """discriminator half: one graph on a static real batch and one static pool draw per discriminator; `vals` / `tot`: its losses.
    `reals`: the real operand of every discriminator -- [real] * n, or with dataaug_APA one static tensor each (`real` is the first);
    `preds` / `lreals`: every loss calculator's `pred_real` / `loss_D_real` inside the graph (what `DiscriminatorGANLoss.update` reads after
    a replay: APA the prediction, dataaug_D_diffusion the loss)"""
    real: torch.Tensor
    fakes: list
    graph: object = None
    vals: list = None
    tot: torch.Tensor = None
    reals: list = None
    preds: list = None
    lreals: list = None


class CUTStepDriver:
    def __init__(self, model):
        self.model, self.drawn_fakes = model, None                   # drawn_fakes: the pool draws of the running step, for compute_D_loss
        self.d_stream = self.gan_stream = self.wg_stream = self.cap_stream = None      # created on first use (`stream`)
        self.g_half = CapturedHalf(model, "jg_graph_G", "JG_GRAPH_G", "generator", "generator graph dropped", "G")
        self.d_half = CapturedHalf(model, "jg_graph_D", "JG_GRAPH_D", "discriminator", "graph dropped", "1",
                                   "HIP_GRAPHS_SAFE is False (HIP initialised before DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 could be set)")

    def stream(self, name):
        """`d_stream` (discriminator half), `gan_stream` (forked GAN branch of compute_G_loss), `wg_stream` or `cap_stream` (the stream the
        generator graphs are captured on), created on first use.  No two of them are the same HIP stream: torch hands its 32 pool streams out
        round-robin to every `torch.cuda.Stream()` of the process, and the per-stream scratch of the launch layer (split-K workspace, zeroed
        rows) is keyed by the raw stream of the launch or of the capture.  The discriminator half and graph B run side by side; when `d_stream`
        happened to be the pool stream graph B was captured on (torch's process-wide default capture stream, before `cap_stream`), the two
        shared one split-K workspace and the generator's gradients came out wrong by orders of magnitude -- one process in 32, by the number
        of streams created before."""
        if getattr(self, name) is None:
            taken = {getattr(self, n).cuda_stream for n in ("d_stream", "gan_stream", "wg_stream", "cap_stream") if getattr(self, n) is not None}
            s = torch.cuda.Stream(device=self.model.device)
            while s.cuda_stream in taken:
                s = torch.cuda.Stream(device=self.model.device)
            setattr(self, name, s)
        return getattr(self, name)

    # ---- the discriminator half under the generator's backward ------------------------------------------------------------
    def early_D(self):
        """The discriminator group's forward + backward reads `fake_B` (detached), `real_B` and the discriminators' weights: nothing the
        generator group's backward or optimizer step writes.  On one GPU it is therefore ENQUEUED on a second HIP stream right after the
        generator group's forward (ordered behind it: spectral-norm power iterations, BatchNorm statistics and the host's pool draws keep
        the reference's order) and runs next to the generator's backward: both are sequences of 10 - 30 us launches that fill a fraction
        of the 256 CUs each.  The discriminators' optimizer step stays where the reference has it, behind a stream join.  Same kernels,
        same operands: results differ from the sequential order only by fp32 atomics ordering.  `jg_early_D=False` / `JG_EARLY_D=0`
        = the sequential driver of BaseModel.  Data parallel (round 5, VERDICT r4 missing #3): the same driver on every rank -- cut_model does
        not opt into `overlap_exchange`, so the gradient all-reduce of every arena is issued by its optimizer step
        (parallel.allreduce_and_step) on the compute stream, AFTER `main.wait_stream(side)`: the side stream never carries a collective and
        the discriminators' gradients are final when their chunks leave.  The generator-half graphs stay single-process (the generator's
        BatchNorm layers all-reduce their batch statistics inside the forward when world_size > 1: a collective inside a capture)."""
        m = self.model
        return (gate(m.opt, "jg_early_D", "JG_EARLY_D") and m.isTrain and m.device.type == "cuda"
                and m.networks_groups == [m.group_G, m.group_D] and not m.group_D.forward_functions and not m.overlap_exchange)

    def wgrad_stream(self):
        """`JG_WGRAD_GROUP_STREAM=1` (A/B): the grouped weight-gradient launches of the generator's backward (ops.deferred_wgrads) leave on a third
        stream every 48 problems instead of on the compute stream at the end.  Measured SLOWER (30.3 vs 29.4 ms/step, same box, everything replayed
        from graphs: the forked branch costs the graph more than the overlap returns): off."""
        return self.stream("wg_stream") if os.environ.get("JG_WGRAD_GROUP_STREAM", "0") == "1" else None

    def draw_pool_fakes(self, side):
        """The history-pool draws of compute_D_loss (`CUTModel.draw_D_fakes`: with dataaug_D_noise the noisy fake batch is formed first, by one
        eager launch on the stream the draws run on; with dataaug_APA every query is followed by that discriminator's `get_random`), made on the MAIN stream before the side stream forks: `ImagePool.query` clones a stored
        image (a view of an earlier generator output, allocated on the main stream) and drops the last reference to it, so on the side
        stream the clone would only be queued when the caching allocator hands the block back to the main stream's pool (ADVICE r4:
        cross-stream use-after-free).  The drawn batches are then marked as in use by the side stream."""
        m = self.model
        if POOL_ON_SIDE:
            # round 6: the draws themselves on the discriminator stream (~40 copy launches per step that graph B no longer queues behind):
            # the pool marks every stored image it reads there (`reader_stream`), the fresh batch is marked here
            for t in self._pool_sources():
                t.record_stream(side)
            side.wait_stream(torch.cuda.current_stream(m.device))
            with torch.cuda.stream(side):
                return m.draw_D_fakes(reader_stream=side)
        fakes, alts = m.draw_D_fakes()
        for f in fakes + (alts or []):
            f.record_stream(side)
        return fakes, alts

    def _pool_sources(self):
        """what `draw_D_fakes` reads of the generator half's outputs: fake_B, or with data_online_context_pixels the framed fake (and its
        noisy copy with dataaug_D_noise)"""
        m = self.model
        if not m.context:
            return [m.fake_B]
        return [m.fake_B_with_context] + ([m.fake_B_with_context_noisy] if m.d_noise > 0.0 else [])

    def optimize_parameters(self):
        """the early-D step; `model.step_driver` says which form of each half ran"""
        m = self.model
        m.niter += 1
        m._ema_fused_this_iter = set()
        gG, gD, its = m.group_G, m.group_D, m.opt.train_iter_size
        m._group_flags(gG)
        main, side = torch.cuda.current_stream(m.device), self.stream("d_stream")
        gst = self.g_from_graph(its)           # forward + losses of the generator group replayed from a hipGraph (None: eager)
        if gst is None:
            for fn in (gG.forward_functions or []) + gG.backward_functions:
                getattr(m, fn)()
        self.drawn_fakes = self.draw_pool_fakes(side)
        try:                               # whatever happens below, a later compute_D_loss must query the pool again, not reuse these
            m.real_B_D.record_stream(side)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                m._group_flags(gD)
                if self.d_from_graph(side, its):
                    m.step_driver = "graph"
                else:
                    m.step_driver = "early"
                    for fn in gD.backward_functions:
                        getattr(m, fn)()
                    for loss in gD.loss_backward:
                        (getattr(m, loss) / its).backward()
        finally:
            self.drawn_fakes = None
        if os.environ.get("JG_DBG_EARLY_D_SYNC"):      # dev (tools/dbg_graph_d.py): the two halves one after the other
            torch.cuda.synchronize()
        m._group_flags(gG)
        if gst is not None:
            gst.bwd.replay()
            m.step_driver += "+graphG"
        else:
            with ops.deferred_wgrads(self.wgrad_stream()):
                for loss in gG.loss_backward:
                    (getattr(m, loss) / its).backward()
        m._group_finish(gG)
        main.wait_stream(side)
        m._group_flags(gD)            # the flags end the step as the sequential driver leaves them
        m._group_finish(gD)
        for obj in m.objects_to_update:
            obj.update(m.niter)
        m.poll_overflow()

    # ---- the generator half as two hipGraphs ------------------------------------------------------------------------------
    def g_from_graph(self, its):
        """`jg_graph_G` (default on with `jg_graph_D`; `JG_GRAPH_G=0` / `1` overrides): the generator group's forward + losses and its
        backward -- ~2500 launches, 35 ms of host enqueue per step at the configs[2] shape, which IS the step time on a host slower than
        the GPU side (336 images/s on the driver's box against 377 here) -- are captured once (third step on) as TWO graphs
        that share a memory pool: graph F = forward_cut + compute_G_loss on static copies of real_A / real_B, graph B = the backward of
        loss_G_tot (retain_graph: its saved activations are F's outputs).  A step replays F, enqueues the discriminator half on the side
        stream (its own graph, `d_from_graph`), replays B under it, and runs the three optimizer launches eagerly (their step
        count and learning rate are host scalars).  What makes this possible: DropPath / Dropout2d scales and the patch ids are drawn
        ON THE DEVICE inside the capture (torch's graph-safe Philox state advances per replay; `torch.randperm` is replaced by rand + topk
        while capturing), the history pools stay outside (the real-image pools before F, the fake pool between F and the discriminator
        half), and every arena's 16-bit working copies are refreshed INSIDE graph F (captured while dirty).  The same two guards as
        for the discriminator half: `HIP_GRAPHS_SAFE`, and a canary -- replay F + B twice from the same RNG state with 8192 eager
        launches in between; losses and the generator's gradient must agree -- after which the touched state (gradient arenas,
        spectral-norm vectors, BatchNorm statistics, RNG offset) is restored.  Returns the graph state or None (eager half)."""
        m = self.model
        if (not self.g_half.ready() or parallel.world_size() > 1 or m.patch_ids_injection is not None
                or getattr(getattr(m._net("G_A"), "rand", None), "source", None) is not None):
            return None
        nets = [m._net(n) for n in m.model_names]
        key = (tuple(m.real_A.shape), tuple(m.real_B.shape), m.real_A.dtype, its, float(m.loss_scale))
        if m.context:                   # the framed shapes: graph F holds static copies of the two with-context images and the frame launch
            key += (tuple(m.real_A_with_context.shape), tuple(m.real_B_with_context.shape), m.d_aug_injection is not None)
        st = self.g_half.get(key, nets, lambda restore: self._g_capture(its, nets, restore))
        if st is None:
            return None
        if m.opt.isTrain:               # the metric pools of forward(): host draws in the reference's order, outside the graph
            m.real_A_pool.store(m.real_A)
            m.real_B_pool.store(m.real_B)
        st.real_A.copy_(m.real_A)
        st.real_B.copy_(m.real_B)
        m.real_A, m.real_B = st.real_A, st.real_B
        if m.context:
            st.ctx_A.copy_(m.real_A_with_context)
            st.ctx_B.copy_(m.real_B_with_context)
            m.real_A_with_context, m.real_B_with_context = st.ctx_A, st.ctx_B
            m.frame_noise_injection()          # parity runs: this step's z of the framed fake into the buffer graph F reads
        st.fwd.replay()
        for n in nets:                     # graph F has just refreshed every trained working copy on the device: the host-side flag follows,
            n.arena._dirty = False         # or the discriminator half would refresh D's copies again on the side stream while graph B reads them
        for k, v in st.outs.items():
            setattr(m, k, v)
        if m.fake_B_pool.pool_size > 0:        # the pool keeps views of what it is handed: not of a buffer the next replay overwrites
            if m.context:                      # (the framed fake, noisy with dataaug_D_noise: CUTModel.draw_D_fakes)
                name = "fake_B_with_context_noisy" if m.d_noise > 0.0 else "fake_B_with_context"
                setattr(m, name, getattr(m, name).clone())
            else:
                m.fake_B = m.fake_B.clone()
        return st

    def _g_capture(self, its, nets, restore):
        m = self.model
        st = GenGraphs(m.real_A.clone(), m.real_B.clone(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph())
        keep_inputs, rng = (m.real_A, m.real_B), torch.cuda.get_rng_state(m.device)
        if m.context:
            st.ctx_A, st.ctx_B = m.real_A_with_context.clone(), m.real_B_with_context.clone()
            keep_ctx = (m.real_A_with_context, m.real_B_with_context)
            m.frame_noise_injection()          # (allocated and filled outside the capture)
        try:
            for n in nets:
                n.arena.ensure_fresh()             # (never-trained working copies: derived now, outside the graph)
                n.arena._dirty = True              # the refresh of every TRAINED working copy belongs to graph F
            m.real_A, m.real_B = st.real_A, st.real_B
            if m.context:
                m.real_A_with_context, m.real_B_with_context = st.ctx_A, st.ctx_B
            with torch.cuda.graph(st.fwd, stream=self.stream("cap_stream"), capture_error_mode="thread_local"):
                ops.zero_pool_reset(m.device, True)          # the zeroed reduction rows of this graph come out of a chunk it clears itself
                m._forward_core()
                m.compute_G_loss()
            names = ["fake", "fake_B", "loss_G_tot", "loss_G_NCE"] + ["loss_G_GAN_" + dn for dn in m.discriminators_names]
            names += [k for k in ("loss_G_supervised", "loss_G_MSE_idt") if k[len("loss_"):] in m.loss_names_G]      # the pixel terms that exist
            if m.context:                   # the frame launch is part of graph F (with dataaug_D_noise: its key draw and the noisy copy too)
                names += ["fake_B_with_context"] + (["fake_B_with_context_noisy"] if m.d_noise > 0.0 else [])
            st.outs = {k: getattr(m, k) for k in names + (["idt_B", "loss_G_NCE_Y"] if m.opt.alg_cut_nce_idt else [])}
            with torch.cuda.graph(st.bwd, pool=st.fwd.pool(), stream=self.stream("cap_stream"), capture_error_mode="thread_local"):
                ops.zero_pool_reset(m.device, True)
                with ops.deferred_wgrads(self.wgrad_stream()):     # the ~190 weight gradients of the generator leave as grouped launches on a forked stream
                    (m.loss_G_tot / its).backward(retain_graph=True)
            ops.zero_pool_reset(m.device)

            def once():
                torch.cuda.set_rng_state(rng, m.device)
                restore()
                st.fwd.replay()
                st.bwd.replay()
                return torch.stack([st.outs["loss_G_tot"].detach().float().reshape(()), m._net("G_A").arena.g.norm()]).clone()

            first = once()
            burst = torch.zeros(64, device=m.device)
            for _ in range(8192):
                burst.add_(1.0)
            second = once()
            # same RNG state, same operands: the two runs differ by the summation order of the fp32 atomics only (measured 2e-4 on the loss,
            # 2e-3 on the gradient norm of a small model); the corruption this guards against shows as NaN or a loss that moves by per cents
            self.g_half.check(first, second, torch.tensor([5e-3, 5e-2], device=first.device), "the generator graphs")
            return st
        finally:                           # passed or failed: the caller's inputs and RNG offset come back, every working copy is stale
            torch.cuda.set_rng_state(rng, m.device)
            m.real_A, m.real_B = keep_inputs
            if m.context:
                m.real_A_with_context, m.real_B_with_context = keep_ctx
            for n in nets:
                n.arena._dirty = True

    # ---- the discriminator half as a hipGraph -----------------------------------------------------------------------------
    def d_from_graph(self, side, its):
        """`jg_graph_D` (default on; `JG_GRAPH_D=0` / `1` overrides the option): the discriminator half -- ~700 launches whose operands
        are two images and the discriminators' arenas -- is captured once (third step on) and replayed.  It holds no host-side random
        draw (the pool queries stay outside), no optimizer step and no host-computed scalar that changes between steps (16-bit
        activations other than fp16: the loss scale is 1).  What it buys is host time: the eager half costs 7.8 ms of enqueue per step,
        and the step's wall time is the enqueue time on hosts slower than the GPU side: 380 images/s on every box instead of 300 - 370
        on the configs[2] shape.

        Two conditions, both checked.  (1) ROCm 7.2's hipGraph replays go wrong when thousands of eager launches run between two
        replays -- its AQL-packet capture keeps the nodes' kernel arguments where later launches overwrite them
        (profiles/r04_graph_replay_probe.txt: the loss of an untouched graph moves after 3000 one-element `add_` launches on another
        stream, NaN gradients after a generator backward).  `DEBUG_CLR_GRAPH_PACKET_CAPTURE=0`, read by the runtime when it
        initialises, switches that path off; `joligen_amd/__init__.py` sets it when the package is imported before the first HIP call
        and records in `HIP_GRAPHS_SAFE` whether it could -- without that the eager half runs.  As a second net the capture is
        followed once by a canary: replay, 8192 tiny eager launches, replay; if the two losses differ the graph is dropped for good
        (with a warning); the canary's side effects (gradient accumulation, spectral-norm power iterations, running statistics) are
        undone from snapshots.  (2) Every tensor the graph reads has to keep its address: the lazily derived tables of the frozen
        feature network (`_FrozenBN.affine`, `_DWWeight.taps`) are refreshed in place for that reason -- re-created, their old storage
        went back to the allocator and the replays read whatever was written there next (found as projected-discriminator logits 1.3 -
        3x too large on a 64 x 64 model; tests/test_gpu_5_cutloss.py::test_cut_step_drivers_agree holds the three drivers together).
        Returns False when the eager path has to run (not enabled, not applicable, capture failed, canary failed)."""
        m = self.model
        if not self.d_half.ready():
            return False
        nets = [m._net(dn) for dn in m.discriminators_names]
        if parallel.world_size() > 1 and any(getattr(mod, "jg_forward_collective", False) or isinstance(mod, torch.nn.SyncBatchNorm)
                                             for n in nets for mod in n.modules()):
            # the side stream (and a captured graph) must never carry a collective: none of today's discriminators has one in its forward --
            # BatchNorm statistics are per rank, as in the reference's DDP default -- a module that adds one marks itself and gets the eager path
            m.step_driver_note = "a discriminator module issues a collective in its forward: discriminator half not captured"
            return False
        real, fake = m.real_B_D, m.fake_B_D        # with data_online_context_pixels: the framed images, and so are the static operands
        key = (tuple(real.shape), real.dtype, tuple(fake.shape), its, float(m.loss_scale))
        st = self.d_half.get(key, nets, lambda restore: self._d_capture(side, its, nets, restore))
        if st is None:
            return False
        fakes, alts = self.drawn_fakes
        if m.d_noise > 0.0 or m.d_apa:      # one eager launch ahead of the replay writes the static real operand(s): no copy on top of it
            m.real_D_operands(alts, outs=st.reals if m.d_apa else st.reals[:1])
        else:
            st.real.copy_(real)
        for dst, f in zip(st.fakes, fakes):
            dst.copy_(f)
        st.graph.replay()
        for dn, pred, lreal in zip(m.discriminators_names, st.preds, st.lreals):      # `update` (after the join) reads THIS graph's replay
            calc = getattr(m, dn + "_loss_calculator")
            calc.pred_real, calc.loss_D_real = pred, lreal
        for dn, val in zip(m.discriminators_names, st.vals):      # published as copies: the next replay overwrites the graph's own
            setattr(m, "loss_D_GAN_" + dn, val.detach().clone())
        m.loss_D_tot = st.tot.detach().clone()
        return True

    def _d_capture(self, side, its, nets, restore):
        m = self.model
        real, fake = m.real_B_D, m.fake_B_D
        st = DiscGraph(real.clone(), [fake.detach().clone() for _ in nets], torch.cuda.CUDAGraph())
        st.reals = [st.real] + [real.clone() for _ in nets[1:]] if m.d_apa else [st.real] * len(nets)
        with torch.cuda.graph(st.graph, stream=side, capture_error_mode="thread_local"):      # other threads (pinned staging, checkpoint writer) may allocate
            ops.zero_pool_reset(m.device, True)
            st.vals, st.tot = m._d_half_body(st.reals, st.fakes, its)
        st.preds = [getattr(m, dn + "_loss_calculator").pred_real for dn in m.discriminators_names]
        st.lreals = [getattr(m, dn + "_loss_calculator").loss_D_real for dn in m.discriminators_names]
        ops.zero_pool_reset(m.device)
        # dataaug_D_diffusion draws a Philox key inside the graph: the canary's two replays start from the same generator state (as the
        # generator half's do), which the caller gets back afterwards
        rng = torch.cuda.get_rng_state(m.device) if getattr(m, "d_diffusion", False) else None
        try:
            return self._d_canary(side, st, restore, rng)
        finally:
            if rng is not None:
                torch.cuda.set_rng_state(rng, m.device)

    def _d_canary(self, side, st, restore, rng):
        m = self.model
        st.graph.replay()
        first = st.tot.detach().clone()
        burst = torch.zeros(64, device=m.device)
        for _ in range(2048):
            burst.add_(1.0)
        with torch.cuda.stream(torch.cuda.default_stream(m.device)):
            for _ in range(6144):
                burst.add_(1.0)
        side.wait_stream(torch.cuda.default_stream(m.device))
        restore()                          # both replays start from the same power-iteration vectors / statistics
        if rng is not None:
            torch.cuda.set_rng_state(rng, m.device)
        st.graph.replay()
        self.d_half.check(first, st.tot.detach().clone(), 1e-3, "an untouched graph", ": export DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before the first HIP call")
        return st
