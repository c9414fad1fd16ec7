"""Worker for test_gpu_wgrad.py::test_mwgrad_het_env_variants, and the
home of the wgrad launch helpers that test file shares with it.

mwgrad_het reads TAC_AMD_WGRAD_XCD (XCD-clustered tile enumeration) and
TAC_AMD_WGRAD_RNRK (128x128 sub-tiled body for M >= 1024 in bf16) once
per process, so each variant needs a fresh process started with the
variables set.  Usage: wgrad_env_worker.py [XCD] [RNRK] -- the names say
which of the two variables the parent must have set to 1; the other must
not be.  Runs every het case with integer operands in both compute dtypes
against the float64 reference of kernel_refs.py, under the plan
het_plan(..., xcd=..., rnrk=...) predicts.  Exits non-zero on any
mismatch."""

import os
import sys

import torch

import kernel_refs as kr

DEV = "cuda:0"
GUARD = 64          # sentinel floats between and around the outputs
ENV = {"XCD": "TAC_AMD_WGRAD_XCD", "RNRK": "TAC_AMD_WGRAD_RNRK"}


class WgOut:
    """dw / db of every problem as views into ONE sentinel-filled flat
    buffer, with GUARD floats before, between and after them."""

    def __init__(self, problems):
        spans, at = [], GUARD
        for p in problems:
            for size in (p.N * p.K, p.N if p.bias else 0):
                spans.append((at, size))
                if size:
                    at += size + GUARD
        self.flat = torch.full((at,), kr.SENTINEL, device=DEV)
        self.spans = spans
        views = [self.flat[o:o + s] for o, s in spans]
        self.dws = [v.view(p.N, p.K) for v, p in zip(views[0::2], problems)]
        self.dbs = views[1::2]          # numel 0: no bias gradient wanted

    def stray_writes(self):
        """Number of guard elements that no longer hold the sentinel."""
        guard = torch.ones(self.flat.numel(), dtype=torch.bool)
        for o, s in self.spans:
            guard[o:o + s] = False
        return int((self.flat.cpu()[guard] != kr.SENTINEL).sum())


def _dev(t):
    return None if t is None else t.to(DEV)


def launch_mwgrad(ext, case, ops):
    """One mwgrad launch for the nz problems of `case`."""
    out = WgOut(case.problems)
    ext.mwgrad([o.dy.to(DEV) for o in ops], [_dev(o.mask) for o in ops],
               [o.x.to(DEV) for o in ops], out.dws, out.dbs, case.M, case.N,
               case.K, case.lddy or case.N, case.ldx or case.K, case.x_off)
    torch.cuda.synchronize()
    return out


def het_args(ops, out):
    ps = [o.prob for o in ops]
    return ([o.dy.to(DEV) for o in ops], [_dev(o.mask) for o in ops],
            [o.x.to(DEV) for o in ops], out.dws, out.dbs,
            [p.M for p in ps], [p.N for p in ps], [p.K for p in ps],
            [p.ld_dy for p in ps], [p.ld_x for p in ps],
            [p.x_off for p in ps])


def launch_het(ext, ops):
    """One mwgrad_het launch for every problem in `ops`."""
    out = WgOut([o.prob for o in ops])
    ext.mwgrad_het(*het_args(ops, out))
    torch.cuda.synchronize()
    return out


def mismatches(name, ops, out, refs):
    """Messages for every dw / db that is not bit-equal to its reference,
    and for stray writes into the guards."""
    msgs = []
    for z, (o, (dw, db, _, _)) in enumerate(zip(ops, refs)):
        msg = kr.describe_mismatch(out.dws[z].cpu().double(), dw)
        if msg:
            msgs.append(f"{name}[{z}] dw: {msg}")
        if o.prob.bias:
            msg = kr.describe_mismatch(out.dbs[z].cpu().double(), db)
            if msg:
                msgs.append(f"{name}[{z}] db: {msg}")
    stray = out.stray_writes()
    if stray:
        msgs.append(f"{name}: {stray} stray writes into the guards")
    return msgs


def split_of(ext, problems):
    return ext.mwgrad_het_adam_split([p.M for p in problems],
                                     [p.N for p in problems],
                                     [p.K for p in problems])


def main(argv):
    want = set(argv)
    if not want or not want <= set(ENV):
        print("usage: wgrad_env_worker.py [XCD] [RNRK]")
        return 2
    for key, var in ENV.items():
        if (os.environ.get(var) == "1") != (key in want):
            print(f"wgrad_env_worker: the parent must start this with {var}"
                  f"{'=1' if key in want else ' unset'}")
            return 2
    xcd, rnrk = "XCD" in want, "RNRK" in want
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.ops import require_extension
    ext = require_extension()
    bad = []
    for case in kr.MWGRAD_HET_CASES:
        ops = kr.wgrad_operands(case.problems, "int")
        refs = kr.wgrad_refs(ops)
        for dtype in ("fp32", "bf16"):
            bf16 = dtype == "bf16"
            Fo.set_compute_dtype(dtype)
            plan = kr.het_plan(case.problems, bf16, xcd=xcd, rnrk=rnrk)
            pinned = kr.HET_PLANS.get((case.name, bf16, xcd, rnrk))
            if pinned is not None and plan != pinned:
                bad.append(f"{case.name} {dtype}: plan {plan} != {pinned}")
            # the host's own split (it knows XCD; the Adam launch it plans
            # for never sub-tiles, so RNRK does not enter)
            host = split_of(ext, case.problems)
            mirror = kr.het_plan(case.problems, bf16, xcd=xcd)[0]
            if host != mirror:
                bad.append(f"{case.name} {dtype}: host split {host}, "
                           f"mirror {mirror}")
            out = launch_het(ext, ops)
            bad += mismatches(f"{case.name} {dtype} plan={plan}", ops, out,
                              refs)
    Fo.set_compute_dtype("fp32")
    for msg in bad:
        print("MISMATCH", msg)
    if bad:
        print(f"wgrad_env_worker: {len(bad)} failures")
        return 1
    print("wgrad_env_worker: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
