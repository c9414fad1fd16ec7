"""Hand-scheduled fused SAC update engine.

Replaces the autograd-recorded update (112 kernels/update, 75% of GPU
time in scalar-staged GEMMs — profiles/r01_baseline_update_profile.md)
with an explicit kernel schedule of 22 launches at batch 64 (21 with the
pi-loss fold switched on, 24 with the q-loss fold switched off, 26 with
the bump and rank-1 folds off as well, 20 with the Adam fold forced on)
built from the multi-problem MFMA kernels in ops/csrc/fused.hip:

 * one Philox counter bump covers the replay draw AND the policy noise;
   it has no launch of its own: gather2/tg_fwd2 key on ctr+1 and the
   launch that computes the q-loss, which runs after both, commits ctr
   and both Adam step counters (TAC_AMD_BUMP_FOLD=0 restores the bump3
   launch);
 * where the small-shape bf16 GEMM runs (batch <= 128, hidden <= 256)
   neither loss has a launch of its own.  The critic phase's masked
   dgrad of the last hidden layer computes the Bellman backup and dq per
   staged row, forms dq (x) w_last in registers (so the K=1 dgrad launch
   goes too), writes dq and that outer product for the wgrad, and its
   block (0, 0, 0) reduces the loss and commits the counters
   (mgemm_r1_qloss; TAC_AMD_QLOSS_FOLD=0 restores qloss2 + the K=1
   launch; needs two hidden layers and the unweighted loss).  The policy
   phase's rank-1 dgrad does the same with the pi-loss (mgemm_r1_piloss;
   off by default, TAC_AMD_PILOSS_FOLD=1 switches it on).  Both are
   decided when a phase is recorded and give the unfolded schedule's
   bits;
 * at world=1 a phase's heterogeneous wgrad launch can apply Adam
   (+polyak, +W^T refresh) itself, replacing the adam_t launch.  By
   default (TAC_AMD_WGRAD_ADAM=auto) it does so where the launch splits
   along M — large batch, or fp32 at batch 64 — and the many-block
   combine kernel carries the update (+6.7% at batch 4096).  Un-split
   (bf16 batch 64) the update would ride in the tile epilogue of a few
   dozen blocks; that measured inside the run-to-run spread on the
   headline, so it needs TAC_AMD_WGRAD_ADAM=1.  =0 never folds; DP runs
   never fold because the all-reduce sits between wgrad and Adam;
 * the pi-phase K=1 dgrad of the critic's last layer is never
   materialised: the next dgrad GEMM forms dqp (x) w_last in registers
   while staging (TAC_AMD_R1_DGRAD=0 restores the K=1 launch);
 * with a prioritized buffer (ReplayBuffer.set_prioritized) the gather
   draws from the ring's sum tree (gather2p), qloss2 runs its
   importance-weighted instantiation and exports the TD errors, and one
   more launch (per_update) writes the new priorities — the default
   launch count plus one; the default schedule is untouched;
 * the replay gather writes states/actions/next-states directly into
   concat-layout buffers (XC = [s|a ; ns|a2], XC2 = [s|pi]) — torch.cat
   never appears;
 * ONE actor forward over 2B stacked rows serves both the Bellman
   backup action (rows B:, on next-states) and the policy action
   (rows :B, on states) — mathematically identical to the reference's
   two independent draws since the rows are disjoint states;
 * both twin critics run per GEMM launch (blockIdx.z);
 * dgrads are fwd-form GEMMs on cached transposed weights (refreshed by
   the launch that applies Adam);
 * wgrads write straight into the FlatAdam gradient buffers;
 * losses are single-block deterministic reductions accumulating into
   device scalars; alpha may live on device and be Adam-updated
   in-graph (learned entropy temperature, BASELINE north star).

The whole schedule is captured into ONE hipGraph — data-parallel runs
record both flat-bucket RCCL all-reduces inside the graph (RCCL supports
captured collectives), with a 3-graph + host-issued-collective fallback
if the communicator refuses capture.  Reference semantics preserved:
update order, losses and polyak follow sac/algorithm.py:115-162,77-81.
"""

import logging
import math
import os
import typing as t

import torch

from ..buffer.replay import ReplayBuffer
from ..models.mlp import Actor, DoubleCritic
from ..optim import FlatAdam
from ..parallel import comm


_log = logging.getLogger(__name__)


class FusedSACEngine:
    def __init__(self, sac, actor: Actor, critic: DoubleCritic,
                 target_critic: DoubleCritic, buffer: ReplayBuffer,
                 pi_opt: FlatAdam, q_opt: FlatAdam,
                 target_flat: torch.Tensor, batch_size: int,
                 device: torch.device, sample: bool = True,
                 capture: bool = True, philox_seed: int = 0):
        from ..ops import require_extension
        self.ext = require_extension()
        self.sac = sac
        self.actor = actor
        self.critic = critic
        self.buffer = buffer
        self.pi_opt = pi_opt
        self.q_opt = q_opt
        self.target_flat = target_flat
        self.device = device
        self.sample = sample
        self.world = comm.num_procs()
        # TAC_AMD_GRAPH_COLL=force exercises the in-graph-collective
        # capture on a 1-rank RCCL communicator (single-GPU testable)
        self._force_coll = (os.environ.get("TAC_AMD_GRAPH_COLL") == "force"
                            and comm.is_initialized())
        self.seed = philox_seed

        B = self.B = batch_size
        O = self.O = buffer.obs_dim
        A = self.A = buffer.act_dim
        OC = self.OC = O + A
        # padded concat-buffer stride (16-float = 64-byte rows): odd
        # widths (Humanoid 393) otherwise force the staging kernels'
        # scalar fallback paths; K stays OC, only strides/offsets pad
        OCp = self.OCp = (OC + 15) & ~15
        self.act_limit = float(actor.act_limit)
        self.lo = float(actor.log_min_std)
        self.hi = float(actor.log_max_std)

        f32 = dict(device=device, dtype=torch.float32)

        # ---- static batch / activation buffers ------------------------
        self.XC = torch.zeros(2 * B, OCp, **f32)   # [s|a ; ns|a2]
        self.XC2 = torch.zeros(B, OCp, **f32)      # [s|pi]
        self.rew = torch.zeros(B, **f32)
        self.done = torch.zeros(B, **f32)
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        # prioritized replay (ReplayBuffer.set_prioritized): the drawn
        # slots, their probabilities and the TD errors qloss2 exports for
        # the priority update — one launch more than the default schedule
        self.per = bool(getattr(buffer, "prioritized", False)) and sample
        if self.per:
            self.idx = torch.zeros(B, dtype=torch.int64, device=device)
            self.pprob = torch.zeros(B, **f32)
            self.td = torch.zeros(B, **f32)

        # actor trunk
        self.a_hidden = [l.out_features for l in actor.layers]
        self.a_act = [torch.zeros(2 * B, h, **f32) for h in self.a_hidden]
        self.hl = torch.zeros(2 * B, 2 * A, **f32)   # [mu | log_std]
        self.prob = torch.zeros(2 * B, A, **f32)
        self.logp = torch.zeros(2 * B, **f32)
        self.dmu = torch.zeros(B, A, **f32)
        self.dls = torch.zeros(B, A, **f32)
        self.da = [torch.zeros(B, h, **f32) for h in self.a_hidden]

        # critic stacks: widths e.g. [h1, h2, 1]
        self.c_w = [l.out_features for l in critic.q1.layers]
        nL = len(self.c_w)

        def cbufs(rows):
            return [[torch.zeros(rows, w, **f32) for w in self.c_w]
                    for _ in range(2)]

        self.t_act = cbufs(B)     # target critic activations
        self.c_act = cbufs(B)     # critic activations (q phase)
        self.p_act = cbufs(B)     # critic activations (pi phase)
        self.dq = [torch.zeros(B, 1, **f32) for _ in range(2)]
        self.dqp = [torch.zeros(B, 1, **f32) for _ in range(2)]
        self.dcp = cbufs(B)       # pi-phase dgrad chain buffers
        self.dc = cbufs(B)        # q-phase dgrad chain buffers
        self.dxc = torch.zeros(B, OCp, **f32)
        self.dxc2 = torch.zeros(B, OCp, **f32)

        # ---- module parameter views -----------------------------------
        def critic_layers(mod):
            return [(l.weight, l.bias) for l in mod.layers]

        self.cw = [critic_layers(critic.q1), critic_layers(critic.q2)]
        self.tw = [critic_layers(target_critic.q1),
                   critic_layers(target_critic.q2)]
        self.aw = [(l.weight, l.bias) for l in actor.layers]
        self.head_w = [(actor.mu_layer.weight, actor.mu_layer.bias),
                       (actor.log_std_layer.weight, actor.log_std_layer.bias)]

        # ---- transposed-weight caches ---------------------------------
        def wt_like(w):
            return torch.zeros(w.shape[1], w.shape[0], **f32)

        self.cwt = [[wt_like(w) for (w, _) in z] for z in self.cw]
        self.awt = [wt_like(w) for (w, _) in self.aw]
        self.hwt = [wt_like(w) for (w, _) in self.head_w]
        self._c_tr_src = [w for z in self.cw for (w, _) in z]
        self._c_tr_dst = [wt for z in self.cwt for wt in z]
        self._a_tr_src = [w for (w, _) in self.aw] + \
            [w for (w, _) in self.head_w]
        self._a_tr_dst = list(self.awt) + list(self.hwt)
        self.ext.transpose_multi(self._c_tr_src, self._c_tr_dst)
        self.ext.transpose_multi(self._a_tr_src, self._a_tr_dst)
        # flat offsets of each weight slab (for the fused Adam+transpose)
        def offs(opt, srcs):
            base = opt.fp.flat.data_ptr()
            end = base + opt.fp.flat.numel() * 4
            out = []
            for w in srcs:
                ptr = w.data_ptr()
                if not (base <= ptr and ptr + w.numel() * 4 <= end):
                    raise RuntimeError(
                        f"engine: weight {tuple(w.shape)} is not a view "
                        "of its optimizer's flat buffer — was the module "
                        "rebound after FlatAdam construction?")
                out.append((ptr - base) // 4)
            return out
        self._c_offs = offs(q_opt, self._c_tr_src)
        self._a_offs = offs(pi_opt, self._a_tr_src)
        # Final-layer dgrad fusion into the loss kernels: measured
        # SLOWER (A/B 4344 vs 4613 upd/s at batch 64) — the single-block
        # outer-product write loses to the 8-block GEMM it replaces.
        # Kept for study via TAC_AMD_LOSS_FUSE=1; default off.
        self._loss_fuse = (os.environ.get("TAC_AMD_LOSS_FUSE") == "1"
                           and B <= 1024 and len(self.c_w) >= 2)

        # whole-MLP fused forward feasibility (LDS budget)
        from ..ops import functional as Fo
        bf16 = Fo.get_compute_dtype() == "bf16"
        self._empty = torch.empty(0, **f32)
        # Whole-MLP fusion measured SLOWER than the layered pipelined
        # GEMMs at both batch 64 (2388 vs 4644 upd/s) and batch 4096
        # (683 vs 777): the layered path's N/M-parallel grid beats the
        # fused kernel's per-block layer serialization.  Kept available
        # for study via TAC_AMD_MLPF=1; default off.
        self.use_mlpf = (
            os.environ.get("TAC_AMD_MLPF") == "1"
            and self.ext.mlp_fwd_fits(OC, list(self.c_w), bf16)
            and self.ext.mlp_fwd_fits(O, list(self.a_hidden) + [2 * A],
                                      bf16)
            and max(self.a_hidden + [2 * A] + self.c_w) <= 256)

        # ---- losses / alpha -------------------------------------------
        self.loss_q_acc = torch.zeros(1, **f32)
        self.loss_pi_acc = torch.zeros(1, **f32)
        self.learn_alpha = bool(getattr(sac, "learn_alpha", False))
        self.alpha_host = float(sac.alpha)
        if self.learn_alpha:
            self.log_alpha = torch.full((1,), math.log(sac.alpha), **f32)
            self.alpha_dev = self.log_alpha.exp()
            self.alpha_m = torch.zeros(1, **f32)
            self.alpha_v = torch.zeros(1, **f32)
            self.alpha_step = torch.zeros(1, dtype=torch.int64,
                                          device=device)
            self.mean_logp = torch.zeros(1, **f32)
            te = getattr(sac, "target_entropy", None)
            self.target_entropy = float(te if te is not None else -A)
        else:
            self.alpha_dev = None
            self.mean_logp = None

        # Side-stream wgrads (overlapping the dgrad chain via captured
        # fork/join events) measured MUCH slower in-graph: A/B 3732 vs
        # 5464 updates/s — the cross-queue dependency overhead dwarfs the
        # ~5 us kernels at this scale.  Kept for study via
        # TAC_AMD_WGRAD_STREAM=1; default off.
        self._use_side = os.environ.get("TAC_AMD_WGRAD_STREAM") == "1"
        # Batch every wgrad of a backward phase into ONE heterogeneous
        # multi-problem launch (+ one phase-wide combine when split-M
        # kicks in at large batch).  TAC_AMD_WGRAD_BATCH=0 disables
        # for A/B.
        self._wgrad_batch = (os.environ.get("TAC_AMD_WGRAD_BATCH", "1")
                             == "1" and not self._use_side)
        self._wjobs: t.List[tuple] = []
        # Adam folded into the phase-wide wgrad launch: only where nothing
        # sits between the wgrad and Adam (single rank, no collective) and
        # the phase's dW/db slices tile the optimizer's flat gradient
        # exactly once (checked per optimizer at the first flush).
        # "auto" (default) folds only launches that split along M, where
        # the combine kernel applies the update; "1" also folds un-split
        # launches (tile epilogue); "0" never folds.
        adam_flag = os.environ.get("TAC_AMD_WGRAD_ADAM", "auto")
        self._wgrad_adam_unsplit = adam_flag == "1"
        self._wgrad_adam = (
            adam_flag != "0"
            and self.world == 1 and not self._force_coll
            # the forced split-graph structure rehearses the
            # data-parallel schedule, which keeps its adam_t launches
            and os.environ.get("TAC_AMD_SPLIT_GRAPHS") != "1"
            and self._wgrad_batch)
        self._adam_fused: t.Dict[int, bool] = {}
        # grad slice -> transposed-weight cache, for the fused W^T refresh
        self._wt_of = {
            w.grad.data_ptr(): wt
            for w, wt in zip(self._c_tr_src + self._a_tr_src,
                             self._c_tr_dst + self._a_tr_dst)}
        # counter bump committed by qloss2 instead of its own launch
        self._bump_fold = os.environ.get("TAC_AMD_BUMP_FOLD", "1") != "0"
        # pi-phase last-layer dgrad as a rank-1 A operand of the next GEMM
        self._r1_dgrad = (
            os.environ.get("TAC_AMD_R1_DGRAD", "1") != "0"
            and len(self.c_w) >= 2 and not self._loss_fuse)
        if self._r1_dgrad and any(self.cwt[z][-1].data_ptr() % 16
                                  for z in range(2)):
            _log.info("engine: rank-1 dgrad operand off (last-layer W^T "
                      "row is not 16-byte aligned); keeping the K=1 launch")
            self._r1_dgrad = False
        # Loss kernels folded into the GEMM that follows them: the critic
        # phase's qloss2 + K=1 dgrad go into the masked dgrad
        # (mgemm_r1_qloss), the policy phase's piloss2 into mgemm_r1
        # (mgemm_r1_piloss).  The flags only ask; each phase decides when
        # it is recorded (_fold_q / _fold_pi), because the folded form
        # exists for the small-shape bf16 kernel alone and both the
        # compute dtype and mgemm_small_mode can change after construction.
        self._qloss_fold_req = (
            os.environ.get("TAC_AMD_QLOSS_FOLD", "1") != "0")
        # The q fold measured +3.9 % on the headline and ships on; the pi
        # fold measured +1.7 % on --mode updates but inside the run-to-run
        # spread on the headline, so it stays behind TAC_AMD_PILOSS_FOLD=1
        # (OPTIMIZATION_LOG.md, "Loss folds").
        self._piloss_fold_req = (
            os.environ.get("TAC_AMD_PILOSS_FOLD", "0") == "1")
        self._qloss_fold = False
        self._piloss_fold = False
        # host-only predicate, no launch: bound here so that it does not
        # count among the launcher calls made through self.ext
        self._fold_ok = self.ext.mgemm_r1_fold_ok
        self._s2 = torch.cuda.Stream()
        self._fork_evs = [torch.cuda.Event() for _ in range(12)]
        self._join_evs = [torch.cuda.Event() for _ in range(4)]
        self._ev_i = 0
        self._join_i = 0

        torch.cuda.synchronize()

        # ---- capture ---------------------------------------------------
        self._graphs = None
        self.graph = None
        if capture:
            self._capture()

    # ------------------------------------------------------------------
    # recorded phases
    # ------------------------------------------------------------------

    def _side(self, fn):
        """Run fn's kernels on the side stream, ordered after the work
        already enqueued on the main stream."""
        if not self._use_side:
            fn()
            return
        ev = self._fork_evs[self._ev_i % len(self._fork_evs)]
        self._ev_i += 1
        ev.record()
        with torch.cuda.stream(self._s2):
            self._s2.wait_event(ev)
            fn()

    def _join_side(self):
        """Main stream waits for everything enqueued on the side stream."""
        if not self._use_side:
            return
        ev = self._join_evs[self._join_i % len(self._join_evs)]
        self._join_i += 1
        with torch.cuda.stream(self._s2):
            ev.record()
        torch.cuda.current_stream().wait_event(ev)

    def _wgrad(self, dys, masks, xs, dws, dbs, M, N, K, lddy, ldx, xoff):
        """Route one wgrad problem group: queue for the phase-wide
        heterogeneous launch, or issue the per-layer mwgrad directly."""
        if self._wgrad_batch:
            for i in range(len(dys)):
                self._wjobs.append((dys[i], masks[i], xs[i], dws[i],
                                    dbs[i], M, N, K, lddy, ldx, xoff))
        else:
            self._side(lambda: self.ext.mwgrad(
                list(dys), list(masks), list(xs), list(dws), list(dbs),
                M, N, K, lddy, ldx, xoff))

    def _adam_covers(self, opt) -> bool:
        """May this phase's wgrad launch carry opt's Adam step?  Decided
        once per optimizer from the queued problems."""
        if not self._wgrad_adam:
            return False
        key = id(opt)
        if key not in self._adam_fused:
            g = opt.fp.flat_grad
            base, ranges = g.data_ptr(), []
            for job in self._wjobs:
                dw, db = job[3], job[4]
                ranges.append(((dw.data_ptr() - base) // 4, dw.numel()))
                ranges.append(((db.data_ptr() - base) // 4, db.numel()))
            why = None
            if not 0 < len(self._wjobs) <= 12:
                why = f"{len(self._wjobs)} wgrad problems (limit 12)"
            elif not self.ext.ranges_tile_exactly(ranges, g.numel()):
                why = ("the phase's dW/db slices do not tile the flat "
                       "gradient exactly once")
            elif not self._wgrad_adam_unsplit and \
                    self.ext.mwgrad_het_adam_split(
                        [j[5] for j in self._wjobs],
                        [j[6] for j in self._wjobs],
                        [j[7] for j in self._wjobs]) <= 1:
                # decided with the compute dtype of the first flush; a
                # later dtype switch only changes which epilogue runs
                why = ("the launch does not split along M "
                       "(TAC_AMD_WGRAD_ADAM=1 folds it anyway)")
            if why:
                _log.info("engine: Adam stays in adam_t for the %d-element "
                          "optimizer: %s", g.numel(), why)
            self._adam_fused[key] = why is None
        return self._adam_fused[key]

    def _wflush(self, opt=None, targ=None, rho=0.0):
        """Issue all queued wgrad problems of this phase in ONE launch;
        with `opt`, the same launch applies its Adam step where allowed
        (see _adam_covers) — the caller then skips adam_t."""
        if not self._wjobs:
            return
        cols = [list(c) for c in zip(*self._wjobs)]
        if opt is not None and self._adam_covers(opt):
            wts = [self._wt_of.get(dw.data_ptr()) for dw in cols[3]]
            self.ext.mwgrad_het_adam(
                *cols, opt.fp.flat, opt.fp.flat_grad, opt.m, opt.v,
                opt.step_t, opt.lr, opt.betas[0], opt.betas[1], opt.eps,
                opt.weight_decay, wts, targ, rho)
        else:
            self.ext.mwgrad_het(*cols)
        self._wjobs = []

    def _fold_q(self) -> bool:
        """Does this recording fold qloss2 and the K=1 dgrad into the
        masked dgrad of the layer below?  Needs a GEMM behind the K=1
        launch (two hidden layers), the unweighted loss, the phase-wide
        wgrad launch (it reads dq and the outer product after the folded
        launch wrote them) and the small-shape kernel."""
        nL = len(self.c_w)
        ok = (self._qloss_fold_req and nL >= 3 and not self.per
              and not self._loss_fuse and self._wgrad_batch
              and all(self.cwt[z][nL - 1].data_ptr() % 16 == 0
                      and self.dc[z][nL - 2].data_ptr() % 16 == 0
                      for z in range(2))
              and self._fold_ok(self.B, self.c_w[nL - 2]))
        self._qloss_fold = bool(ok)
        return self._qloss_fold

    def _fold_pi(self) -> bool:
        """Does this recording fold piloss2 into the rank-1 dgrad GEMM?"""
        nL = len(self.c_w)
        ok = (self._piloss_fold_req and self._r1_dgrad
              and not self._loss_fuse
              and self._fold_ok(self.B, self.c_w[nL - 2]))
        self._piloss_fold = bool(ok)
        return self._piloss_fold

    def _mg(self, xs, ws, bs, ys, masks, M, N, K, lda, ldy, relu,
            xs2=None, ws2=None, masks2=None, K2=0, x_off=0, x2_off=0,
            x_offs=None):
        self.ext.mgemm(xs, ws, bs, ys, masks, M, N, K, lda, ldy, relu,
                       xs2 or [], ws2 or [], masks2 or [], K2, x_off,
                       x2_off, x_offs or [])

    def _critic_fwd(self, x_src, x_off, weights, acts, lda,
                    need_hidden_acts=True):
        """Twin-critic forward; acts[z][i] filled.  Final layer no relu."""
        B = self.B
        nL = len(self.c_w)
        if self.use_mlpf:
            e = self._empty
            act_arg = [
                [acts[z][i] if (need_hidden_acts or i == nL - 1) else e
                 for i in range(nL)] for z in range(2)]
            self.ext.mlp_fwd_fused(
                x_src, x_off, lda, B, self.OC,
                [[weights[z][i][0] for i in range(nL)] for z in range(2)],
                [[e] * nL for _ in range(2)],
                [[weights[z][i][1] for i in range(nL)] for z in range(2)],
                [[e] * nL for _ in range(2)],
                act_arg, list(self.c_w), [1 << 30] * nL,
                (1 << (nL - 1)) - 1)
            return
        x = [x_src, x_src]
        k = self.OC
        src_off = x_off
        src_lda = lda
        for i in range(nL):
            relu = i + 1 < nL
            self._mg(x, [weights[z][i][0] for z in range(2)],
                     [weights[z][i][1] for z in range(2)],
                     [acts[z][i] for z in range(2)], [None, None],
                     B, self.c_w[i], k, src_lda, self.c_w[i], relu,
                     x_off=src_off)
            x = [acts[0][i], acts[1][i]]
            k = self.c_w[i]
            src_off = 0
            src_lda = k

    def _gather(self, ctr_add: int):
        """One-launch replay sample + gather into the concat buffers.  An
        n-step buffer (ReplayBuffer.set_n_step) takes the n-step kernel:
        same index draw and layout, rew/done carry the discounted reward
        sum and the effective done, so the rest of the schedule — and
        the launch count — is the same.  A prioritized buffer takes
        gather2p (either n)."""
        ext, buf, B = self.ext, self.buffer, self.B
        if self.per:
            # stratified draw from the sum tree, same Philox keying; the
            # n-step fields are placeholders while n_step == 1
            nstep = buf.n_step > 1
            ext.gather2p(buf.state, buf.actions, buf.rewards,
                         buf.next_state, buf.done,
                         buf.episode_end if nstep else buf.done,
                         buf._size_dev,
                         buf._ptr_dev if nstep else buf._size_dev,
                         buf._per_tree, self.ctr, self.seed, buf.n_step,
                         buf.gamma, self.XC, self.XC2, self.rew, self.done,
                         self.idx, self.pprob, None, B, ctr_add)
        elif buf.n_step > 1:
            ext.gather2n(buf.state, buf.actions, buf.rewards,
                         buf.next_state, buf.done, buf.episode_end,
                         buf._size_dev, buf._ptr_dev, self.ctr, self.seed,
                         buf.n_step, buf.gamma, self.XC, self.XC2, self.rew,
                         self.done, B, ctr_add)
        else:
            ext.gather2(buf.state, buf.actions, buf.rewards, buf.next_state,
                        buf.done, buf._size_dev, self.ctr, self.seed,
                        self.XC, self.XC2, self.rew, self.done, B, ctr_add)

    def _phase_critic(self):
        ext = self.ext
        B, O, A, OC = self.B, self.O, self.A, self.OC
        # the replay/noise counter AND both Adam step counters advance
        # once per update: either one launch up front, or (folded) the
        # readers key on ctr+1 and qloss2 commits all three — both Adam
        # applications run after it on the same stream
        fold = self._bump_fold
        ctr_add = 1 if fold else 0
        if not fold:
            ext.bump3(self.ctr, self.q_opt.step_t, self.pi_opt.step_t)
        if self.sample:
            self._gather(ctr_add)

        # actor forward over stacked 2B rows of XC[:, :O]
        (wm, bm), (wl, bl) = self.head_w
        if self.use_mlpf:
            e = self._empty
            nT = len(self.aw)
            ws = [[w for (w, _) in self.aw] + [wm]]
            whis = [[e] * nT + [wl]]
            bs = [[b for (_, b) in self.aw] + [bm]]
            bhis = [[e] * nT + [bl]]
            acts = [list(self.a_act) + [self.hl]]
            widths = list(self.a_hidden) + [2 * A]
            splits = [1 << 30] * nT + [A]
            relu_mask = (1 << nT) - 1
            ext.mlp_fwd_fused(self.XC, 0, OC, 2 * B, O, ws, whis, bs,
                              bhis, acts, widths, splits, relu_mask)
        else:
            x, k, lda, off = self.XC, O, self.OCp, 0
            for i, (w, b) in enumerate(self.aw):
                self._mg([x], [w], [b], [self.a_act[i]], [None], 2 * B,
                         self.a_hidden[i], k, lda, self.a_hidden[i], True,
                         x_off=off)
                x, k, lda, off = self.a_act[i], self.a_hidden[i], \
                    self.a_hidden[i], 0
            self._mg([x, x], [wm, wl], [bm, bl],
                     [self.hl, self.hl[:, A:]],
                     [None, None], 2 * B, A, k, lda, 2 * A, False)
        # pi rows :B -> XC2[:, O:], a2 rows B: -> XC[B:, O:]
        ext.tg_fwd2(self.hl, self.XC2, O, self.XC, B * self.OCp + O,
                    B, self.logp, self.prob, self.ctr, self.seed,
                    self.act_limit, self.lo, self.hi, ctr_add)

        # target critic on (ns, a2) = XC rows B: AND the live critic on
        # (s, a) = XC rows :B — same shapes, one 4-problem launch per layer
        if not self.use_mlpf:
            nLc = len(self.c_w)
            xs4 = [self.XC] * 4
            offs4 = [B * self.OCp, B * self.OCp, 0, 0]
            k = OC
            lda = self.OCp
            for i in range(nLc):
                relu = i + 1 < nLc
                self._mg(xs4,
                         [self.tw[0][i][0], self.tw[1][i][0],
                          self.cw[0][i][0], self.cw[1][i][0]],
                         [self.tw[0][i][1], self.tw[1][i][1],
                          self.cw[0][i][1], self.cw[1][i][1]],
                         [self.t_act[0][i], self.t_act[1][i],
                          self.c_act[0][i], self.c_act[1][i]],
                         [None] * 4, B, self.c_w[i], k, lda, self.c_w[i],
                         relu, x_offs=offs4)
                xs4 = [self.t_act[0][i], self.t_act[1][i],
                       self.c_act[0][i], self.c_act[1][i]]
                offs4 = [0, 0, 0, 0]
                k = self.c_w[i]
                lda = k
        else:
            self._critic_fwd(self.XC, B * self.OCp, self.tw, self.t_act,
                             self.OCp,
                             need_hidden_acts=False)
            self._critic_fwd(self.XC, 0, self.cw, self.c_act, self.OCp)

        nL = len(self.c_w)
        q = [self.c_act[z][nL - 1] for z in range(2)]
        qt = [self.t_act[z][nL - 1] for z in range(2)]
        # final-layer dgrad (K=1 outer product) fuses into the loss kernel
        fuse = self._loss_fuse
        bump = ((self.ctr, self.q_opt.step_t, self.pi_opt.step_t)
                if self._bump_fold else (None, None, None))
        # importance-weighted instantiation for a prioritized buffer; beta
        # is a device scalar, so a captured graph sees its annealing
        buf = self.buffer
        per = ((self.pprob, buf._size_dev, buf._beta_dev, self.td)
               if self.per else ())
        # folded: no loss launch and no K=1 launch here — the masked
        # dgrad below computes dq, the outer product and the loss itself
        qfold = self._fold_q()
        if not qfold:
            ext.qloss2(q[0], q[1], qt[0], qt[1], self.logp[B:], self.rew,
                       self.done, self.alpha_dev, self.alpha_host,
                       self.loss_q_acc, self.dq[0], self.dq[1], B,
                       self.sac.gamma, self.sac.reward_scale,
                       self.cwt[0][nL - 1] if fuse else None,
                       self.cwt[1][nL - 1] if fuse else None,
                       self.dc[0][nL - 2] if fuse else None,
                       self.dc[1][nL - 2] if fuse else None,
                       self.c_w[nL - 2] if fuse else 0, *bump, *per)
        if self.per:
            # new priorities from this batch's TD errors, ahead of
            # everything that can precede the next gather
            ext.per_update(buf._per_tree, buf.max_size, self.idx, self.td,
                           buf.per_alpha, buf.per_eps, buf._max_priority)

        # critic backward (wgrad into flat grads; dgrad via cached W^T)
        d = self.dq
        for i in range(nL - 1, -1, -1):
            relu_mask = i + 1 < nL   # incoming d is post-relu of layer i?
            masks = [self.c_act[z][i] if relu_mask else None
                     for z in range(2)]
            if i > 0:
                x_in = [self.c_act[z][i - 1] for z in range(2)]
                ldx, xoff = self.c_w[i - 1], 0
            else:
                x_in = [self.XC, self.XC]
                ldx, xoff = self.OCp, 0
            self._wgrad(list(d), list(masks), list(x_in),
                        [self.cw[z][i][0].grad for z in range(2)],
                        [self.cw[z][i][1].grad for z in range(2)],
                        B, self.c_w[i],
                        (self.c_w[i - 1] if i > 0 else OC),
                        self.c_w[i], ldx, xoff)
            if i > 0:
                if i == nL - 1 and (fuse or qfold):
                    pass  # dy2 comes from the loss kernel / the next GEMM
                elif i == nL - 2 and qfold:
                    ext.mgemm_r1_qloss(
                        q[0], q[1], qt[0], qt[1], self.logp[B:], self.rew,
                        self.done, self.alpha_dev, self.alpha_host,
                        self.loss_q_acc, self.dq[0], self.dq[1],
                        self.sac.gamma, self.sac.reward_scale, *bump,
                        [self.cwt[z][nL - 1] for z in range(2)],
                        [self.cwt[z][i] for z in range(2)],
                        [self.dc[z][i - 1] for z in range(2)], masks,
                        [self.dc[z][i] for z in range(2)],
                        B, self.c_w[i - 1], self.c_w[i], self.c_w[i - 1])
                else:
                    self._mg(d, [self.cwt[z][i] for z in range(2)],
                             [None, None],
                             [self.dc[z][i - 1] for z in range(2)],
                             masks, B, self.c_w[i - 1], self.c_w[i],
                             self.c_w[i], self.c_w[i - 1], False)
                d = [self.dc[z][i - 1] for z in range(2)]
        # critic grads must be complete before all-reduce / Adam; at
        # world=1 the same launch applies Adam + polyak + W^T refresh
        # (every critic dgrad that reads the W^T caches is already queued
        # ahead of it on this stream)
        self._wflush(self.q_opt, self.target_flat, self.sac.polyak)
        self._join_side()

    def _phase_policy(self):
        ext = self.ext
        B, O, A, OC = self.B, self.O, self.A, self.OC
        # fused Adam + transposed-weight refresh (step already bumped) —
        # unless the critic wgrad launch already applied it
        qo = self.q_opt
        if not self._adam_fused.get(id(qo), False):
            ext.adam_t(qo.fp.flat, qo.fp.flat_grad, qo.m, qo.v, qo.step_t,
                       qo.lr, qo.betas[0], qo.betas[1], qo.eps,
                       qo.weight_decay, self._c_offs, self._c_tr_dst,
                       self.target_flat, self.sac.polyak)

        # critic on (s, pi) = XC2 with the UPDATED critic
        self._critic_fwd(self.XC2, 0, self.cw, self.p_act, self.OCp)
        nL = len(self.c_w)
        qp = [self.p_act[z][nL - 1] for z in range(2)]
        fuse = self._loss_fuse
        # folded: the rank-1 GEMM below computes dqp and the loss itself
        pfold = self._fold_pi()
        if not pfold:
            ext.piloss2(qp[0], qp[1], self.logp[:B], self.alpha_dev,
                        self.alpha_host, self.loss_pi_acc, self.mean_logp,
                        self.dqp[0], self.dqp[1], B,
                        self.cwt[0][nL - 1] if fuse else None,
                        self.cwt[1][nL - 1] if fuse else None,
                        self.dcp[0][nL - 2] if fuse else None,
                        self.dcp[1][nL - 2] if fuse else None,
                        self.c_w[nL - 2] if fuse else 0)

        def r1_gemm(cols, rows, ws, ys, masks, M, N, K, ldy):
            if pfold:
                ext.mgemm_r1_piloss(
                    qp[0], qp[1], self.logp[:B], self.alpha_dev,
                    self.alpha_host, self.loss_pi_acc, self.mean_logp,
                    cols[0], cols[1], rows, ws, ys, masks, M, N, K, ldy)
            else:
                ext.mgemm_r1(cols, rows, ws, ys, masks, M, N, K, ldy)

        # critic dgrad chain only (frozen critic).  The last layer's
        # dgrad is the outer product dqp (x) w_last (K=1): with r1 it is
        # never written — the next GEMM forms it while staging its A tile
        d = self.dqp
        r1 = None
        for i in range(nL - 1, 0, -1):
            masks = [self.p_act[z][i] if i + 1 < nL else None
                     for z in range(2)]
            if i == nL - 1 and fuse:
                d = [self.dcp[z][i - 1] for z in range(2)]
                continue
            if i == nL - 1 and self._r1_dgrad:
                r1 = (list(self.dqp),
                      [self.cwt[z][nL - 1] for z in range(2)])
                continue
            if r1 is not None:
                r1_gemm(r1[0], r1[1],
                        [self.cwt[z][i] for z in range(2)],
                        [self.dcp[z][i - 1] for z in range(2)], masks,
                        B, self.c_w[i - 1], self.c_w[i], self.c_w[i - 1])
                r1 = None
            else:
                self._mg(d, [self.cwt[z][i] for z in range(2)],
                         [None, None],
                         [self.dcp[z][i - 1] for z in range(2)], masks,
                         B, self.c_w[i - 1], self.c_w[i], self.c_w[i],
                         self.c_w[i - 1], False)
            d = [self.dcp[z][i - 1] for z in range(2)]
        # layer 0: per-critic dxc slabs in one z=2 launch; tg_bwd2 sums
        # them on read (measured faster than the serial two-pass sum2)
        masks0 = [self.p_act[z][0] for z in range(2)]
        if r1 is not None:   # single hidden layer: layer 0 consumes it
            r1_gemm(r1[0], r1[1], [self.cwt[z][0] for z in range(2)],
                    [self.dxc, self.dxc2], masks0, B, OC, self.c_w[0],
                    self.OCp)
        else:
            self._mg(d, [self.cwt[z][0] for z in range(2)], [None, None],
                     [self.dxc, self.dxc2], masks0,
                     B, OC, self.c_w[0], self.c_w[0], self.OCp, False)

        # actor backward
        ext.tg_bwd2(self.dxc, O, self.dxc2, self.alpha_dev,
                    self.alpha_host, self.hl, self.prob, self.dmu,
                    self.dls, B, self.act_limit, self.lo, self.hi)
        h_last = self.a_hidden[-1]
        a_last = self.a_act[-1]
        (wm, bm), (wl, bl) = self.head_w
        self._wgrad([self.dmu, self.dls], [None, None], [a_last, a_last],
                    [wm.grad, wl.grad], [bm.grad, bl.grad],
                    B, A, h_last, A, h_last, 0)
        self._mg([self.dmu], [self.hwt[0]], [None], [self.da[-1]], [None],
                 B, h_last, A, A, h_last, False,
                 xs2=[self.dls], ws2=[self.hwt[1]], masks2=[None], K2=A)

        d = self.da[-1]
        for i in range(len(self.aw) - 1, -1, -1):
            mask = self.a_act[i]
            if i > 0:
                x_in, ldx, xoff = self.a_act[i - 1], self.a_hidden[i - 1], 0
                kin = self.a_hidden[i - 1]
            else:
                x_in, ldx, xoff = self.XC, self.OCp, 0
                kin = O
            (w, b) = self.aw[i]
            self._wgrad([d], [mask], [x_in], [w.grad], [b.grad],
                        B, self.a_hidden[i], kin, self.a_hidden[i],
                        ldx, xoff)
            if i > 0:
                self._mg([d], [self.awt[i]], [None], [self.da[i - 1]],
                         [mask], B, self.a_hidden[i - 1], self.a_hidden[i],
                         self.a_hidden[i], self.a_hidden[i - 1], False)
                d = self.da[i - 1]
        # actor grads must be complete before all-reduce / Adam (same
        # launch applies it at world=1; no polyak for the actor)
        self._wflush(self.pi_opt)
        self._join_side()

    def _phase_finish(self):
        ext = self.ext
        po = self.pi_opt
        if not self._adam_fused.get(id(po), False):
            ext.adam_t(po.fp.flat, po.fp.flat_grad, po.m, po.v, po.step_t,
                       po.lr, po.betas[0], po.betas[1], po.eps,
                       po.weight_decay, self._a_offs, self._a_tr_dst,
                       None, 0.0)
        # polyak is fused into the critic Adam (see _phase_policy)
        if self.learn_alpha:
            ext.alpha_update(self.log_alpha, self.alpha_dev, self.alpha_m,
                             self.alpha_v, self.alpha_step, self.mean_logp,
                             self.target_entropy, 3e-4)

    # ------------------------------------------------------------------

    def _reduce(self, opt, in_graph: bool = False):
        if self.world > 1 or self._force_coll:
            if in_graph:
                comm.allreduce_grads_capturable(opt.fp.flat_grad)
            else:
                comm.allreduce_grads(opt.fp.flat_grad)

    def _run_once(self):
        self._phase_critic()
        self._reduce(self.q_opt)
        self._phase_policy()
        self._reduce(self.pi_opt)
        self._phase_finish()

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run_once()
        torch.cuda.current_stream().wait_stream(s)

        # TAC_AMD_SPLIT_GRAPHS=1 forces the data-parallel 3-graph
        # structure at world=1 so the multi-GPU capture path is testable
        # on a single GPU
        split = (self.world > 1 or self._force_coll
                 or os.environ.get("TAC_AMD_SPLIT_GRAPHS") == "1")
        # Default data-parallel fast path: record BOTH flat-bucket RCCL
        # all-reduces inside ONE hipGraph — one replay per update, no
        # host round-trips between the three phases (xGMI collectives
        # at these sub-MB payloads are latency-bound; so is the host).
        # Falls back to 3 graphs + host-issued collectives if capture
        # of the communicator is refused.
        # TAC_AMD_SPLIT_GRAPHS=1 takes precedence over the in-graph
        # collective branch: the split structure is reachable
        # without also having to set TAC_AMD_GRAPH_COLL=0
        coll_in_graph = ((self.world > 1 or self._force_coll)
                         and comm.backend_name() == "nccl"
                         and os.environ.get("TAC_AMD_GRAPH_COLL", "1")
                         != "0"
                         and os.environ.get("TAC_AMD_SPLIT_GRAPHS") != "1")
        if coll_in_graph:
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._phase_critic()
                    self._reduce(self.q_opt, in_graph=True)
                    self._phase_policy()
                    self._reduce(self.pi_opt, in_graph=True)
                    self._phase_finish()
                self.graph = g
                # arm the first-replay watchdog at real world>1 (see
                # comm.guarded_replay; world=1 force-capture is already
                # hardware-tested every round)
                self._guard_first_replay = self.world > 1
                return
            except Exception as e:  # pragma: no cover - fallback path
                import logging
                logging.getLogger(__name__).warning(
                    "in-graph collective capture failed (%s); "
                    "falling back to split graphs", e)
        if not split:
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self._phase_critic()
                self._phase_policy()
                self._phase_finish()
        else:
            try:
                g1 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g1):
                    self._phase_critic()
                g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g2, pool=g1.pool()):
                    self._phase_policy()
                g3 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g3, pool=g1.pool()):
                    self._phase_finish()
                self._graphs = (g1, g2, g3)
            except Exception as e:  # pragma: no cover - last-resort path
                import logging
                logging.getLogger(__name__).warning(
                    "split-graph capture failed (%s); running the fused "
                    "schedule uncaptured", e)
                self._graphs = None

    def step(self):
        if self.graph is not None:
            if getattr(self, "_guard_first_replay", False):
                self._guard_first_replay = False
                comm.guarded_replay(self.graph)
                return
            self.graph.replay()
        elif self._graphs is not None:
            g1, g2, g3 = self._graphs
            g1.replay()
            self._reduce(self.q_opt)
            g2.replay()
            self._reduce(self.pi_opt)
            g3.replay()
        else:
            self._run_once()

    def read_and_reset_losses(self, n_updates: int):
        if n_updates <= 0:
            return 0.0, 0.0
        lq = float(self.loss_q_acc.item()) / n_updates
        lp = float(self.loss_pi_acc.item()) / n_updates
        self.loss_q_acc.zero_()
        self.loss_pi_acc.zero_()
        return lq, lp

    # -- test helper ----------------------------------------------------

    def load_batch(self, s, a, r, ns, d):
        """Write a batch directly into the static buffers (sample=False
        parity tests)."""
        B, O = self.B, self.O
        self.XC[:B, :O] = s
        self.XC[:B, O:self.OC] = a
        self.XC[B:, :O] = ns
        self.XC2[:, :O] = s
        self.rew.copy_(r)
        self.done.copy_(d)
