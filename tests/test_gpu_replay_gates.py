"""The host gate shared by the six replay gather bindings
(replay_draw.h::gather_gate): replay_sample_into / _n / _p write flat batch
tensors, gather2 / gather2n / gather2p the update engine's concat buffers.

Every binding is called once with good operands and then with one operand
wrong at a time.  Each wrong operand is refused by the host before anything
is launched, so the call raises RuntimeError, every output still holds the
sentinel it was filled with and the Philox counter is unchanged — the flat
bindings bump it only after the gate."""

import pytest
import torch

import kernel_refs as kr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP, OBS, ACT, B = 48, 3, 2, 8
LDC = 8
SEED, GAMMA, CTR0 = 5, 0.99, 11
TREE_LEN = 64 + 64          # root level and 48 leaves, each padded to 64
NSTEP = {"replay_sample_into_n", "replay_sample_into_p", "gather2n",
         "gather2p"}
FLAT = {"replay_sample_into", "replay_sample_into_n", "replay_sample_into_p"}
BINDINGS = sorted(FLAT) + ["gather2", "gather2n", "gather2p"]


@pytest.fixture(scope="module")
def ext():
    from torch_actor_critic_amd.ops import require_extension
    return require_extension()


def _operands():
    f = lambda *s: torch.rand(*s, device=DEV)
    i = lambda v: torch.full((1,), v, dtype=torch.int64, device=DEV)
    s = lambda *shape: torch.full(shape, kr.SENTINEL, device=DEV)
    tree = torch.zeros(TREE_LEN, device=DEV)
    tree[0] = CAP
    tree[64:64 + CAP] = 1.0
    return dict(
        state=f(CAP, OBS), act=f(CAP, ACT), rew=f(CAP), nstate=f(CAP, OBS),
        done=torch.zeros(CAP, device=DEV), ep_end=torch.zeros(CAP, device=DEV),
        size_dev=i(CAP), ptr_dev=i(0), tree=tree, ctr=i(CTR0), n=3,
        os=s(B, OBS), oa=s(B, ACT), ons=s(B, OBS), xc=s(2 * B, LDC),
        xc2=s(B, LDC), orew=s(B), od=s(B), oprob=s(B),
        oidx=torch.full((B,), -7, dtype=torch.int64, device=DEV))


OUTPUTS = ("os", "oa", "ons", "xc", "xc2", "orew", "od", "oprob")


def _call(ext, name, o):
    ring = (o["state"], o["act"], o["rew"], o["nstate"], o["done"])
    nring = ring + (o["ep_end"], o["size_dev"], o["ptr_dev"])
    flat = (o["os"], o["oa"], o["orew"], o["ons"], o["od"])
    cat = (o["xc"], o["xc2"], o["orew"], o["od"])
    if name == "replay_sample_into":
        ext.replay_sample_into(*ring, o["size_dev"], o["ctr"], SEED, *flat)
    elif name == "replay_sample_into_n":
        ext.replay_sample_into_n(*nring, o["ctr"], SEED, o["n"], GAMMA, *flat)
    elif name == "replay_sample_into_p":
        ext.replay_sample_into_p(*nring, o["tree"], o["ctr"], SEED, o["n"],
                                 GAMMA, *flat, o["oidx"], o["oprob"])
    elif name == "gather2":
        ext.gather2(*ring, o["size_dev"], o["ctr"], SEED, *cat, B, 0)
    elif name == "gather2n":
        ext.gather2n(*nring, o["ctr"], SEED, o["n"], GAMMA, *cat, B, 0)
    else:
        ext.gather2p(*nring, o["tree"], o["ctr"], SEED, o["n"], GAMMA, *cat,
                     o["oidx"], o["oprob"], None, B, 0)


def _bad_operands(name):
    """(label, operand, wrong value) — one wrong operand per case."""
    s = lambda *shape: torch.full(shape, kr.SENTINEL, device=DEV)
    wide = torch.rand(CAP, 2 * OBS, device=DEV)   # [:, ::2]: sizes right
    cases = [
        ("float64 ring field",
         "state", torch.rand(CAP, OBS, device=DEV, dtype=torch.float64)),
        ("non-contiguous ring field", "nstate", wide[:, ::2]),
        ("rew one short", "rew", torch.rand(CAP - 1, device=DEV)),
        ("int32 size_dev", "size_dev",
         torch.full((1,), CAP, dtype=torch.int32, device=DEV)),
    ]
    if name in NSTEP:
        cases += [("n = 0", "n", 0), ("n = 65", "n", 65)]
    if name in FLAT:
        cases += [("os too wide", "os", s(B, OBS + 1))]
    else:
        cases += [
            ("xc one row short", "xc", s(2 * B - 1, LDC)),
            ("xc narrower than obs + act", ("xc", "xc2"),
             (s(2 * B, OBS + ACT - 1), s(B, OBS + ACT - 1))),
            ("xc2 of another width", "xc2", s(B, LDC + 1)),
        ]
    if name.endswith("p"):
        cases += [("tree one short", "tree",
                   torch.zeros(TREE_LEN - 1, device=DEV))]
    return cases


@pytest.mark.parametrize("name", BINDINGS)
def test_gather_gate(ext, name):
    o = _operands()
    _call(ext, name, o)
    torch.cuda.synchronize()
    assert int(o["ctr"]) == CTR0 + (name in FLAT)
    rows = o["os"] if name in FLAT else o["xc"][:B, :OBS + ACT]
    assert not bool((rows == kr.SENTINEL).any())
    assert not bool((o["orew"] == kr.SENTINEL).any())

    for label, key, wrong in _bad_operands(name):
        o = _operands()
        if isinstance(key, tuple):
            o.update(zip(key, wrong))
        else:
            o[key] = wrong
        with pytest.raises(RuntimeError):
            _call(ext, name, o)
        torch.cuda.synchronize()
        assert int(o["ctr"]) == CTR0, label
        for out in OUTPUTS:
            assert bool((o[out] == kr.SENTINEL).all()), (label, out)
        assert bool((o["oidx"] == -7).all()), label
