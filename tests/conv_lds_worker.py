"""Worker for test_gpu_conv_exact.py::test_conv_fwd_lds_variant_child_process.

conv2d_fwd reads TAC_AMD_CONV_LDS once, at the first conv call of the
process, so the LDS-subimage forward variant needs a fresh process
started with TAC_AMD_CONV_LDS=1.  Runs the three compiled-family exact
forward cases through that variant, plus one fallback geometry that must
silently take the normal kernel, in both compute dtypes, against the
float64 references of kernel_refs.py.  Exits non-zero on any mismatch."""

import os
import sys

import torch

import kernel_refs as kr

DEV = "cuda:0"


def main():
    if os.environ.get("TAC_AMD_CONV_LDS") != "1":
        print("conv_lds_worker: TAC_AMD_CONV_LDS=1 must be set by the parent")
        return 2
    from torch_actor_critic_amd.ops import functional as Fo
    from torch_actor_critic_amd.ops import require_extension
    ext = require_extension()
    bad = 0
    for geom in kr.CONV_KNOWN + kr.CONV_FALLBACK[:1]:
        S = geom[7]
        sets = [kr.conv_operands(geom, "int", z) for z in range(2)]
        for dtype in ("fp32", "bf16"):
            Fo.set_compute_dtype(dtype)
            for bias in (True, False):
                for relu in (False, True):
                    ys = ext.conv2d_fwd_multi(
                        [o.x.to(DEV) for o in sets],
                        [o.w.to(DEV) for o in sets],
                        [o.b.to(DEV) if bias else None for o in sets],
                        S, relu)
                    for z, (o, y) in enumerate(zip(sets, ys)):
                        ref, _ = kr.conv_fwd_ref(
                            o.x, o.w, o.b if bias else None, S, relu)
                        msg = kr.describe_mismatch(y.cpu().double(), ref)
                        if msg:
                            bad += 1
                            print(f"MISMATCH {kr.conv_id(geom)} {dtype} "
                                  f"bias={bias} relu={relu} [{z}]: {msg}")
    Fo.set_compute_dtype("fp32")
    if bad:
        print(f"conv_lds_worker: {bad} mismatching outputs")
        return 1
    print("conv_lds_worker: OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
