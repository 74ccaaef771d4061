"""-m gpu: the recurrent PPO update inside the engine (mqe_ppo_grad with MQE_PPO_BPTT; csrc/kernels_bptt.hpp: k_bptt_grad, k_bptt_ln_grad,
k_bptt_expand; HipEngine.ppo_grad / ppo_update(chunk_length=)): (1) the gradient against the float64 twin within K_GPU 2^-24 S_n (tests/bptt_ref.py)
over cell widths, depths, norms, chunk lengths, chunk counts at the tile edges, an index list and a range; (2) more tiles than workgroups; (3) value
normalisation, and chunk numbers outside the trajectory, which both paths clamp; (4) determinism, every element written, refusals; (5) a real rollout end to end.  go1gate, D = 16, A' = 2.

THE STATISTICS' BOUNDS (derived; e_p and e_v are the largest per-sample deviations of the float32 torch twin's logp and value from float64 on the same
chunks, the yardstick of tests/gru_ref.py, and the kernel is allowed 4 x them): the clip share is exact on kink-free inputs; the approximate KL is a
mean of logp_old - logp, so it moves by at most 4 e_p; L_pi = -ratio adv away from the clip (a clipped sample is constant) moves by at most
mean(|adv| ratio) (exp(4 e_p) - 1); L_v is a maximum of two squares whose arguments move by at most 4 e_v each: mean(2 |d| + 4 e_v) 4 e_v with |d|
the larger of the two arguments; each plus 2^-22 of its own magnitude for the float32 sum and store."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import bptt_ref as ref
import gru_ref
import ppo_ref
import value_norm_ref as vnref
from mqe.engine import abi
from test_rollout_gpu import engine, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

D = 16
_HANDLES, _SYNTH = {}, {}


def handle(N, **kw):
    key = (N, tuple(sorted(kw.items())))
    if key not in _HANDLES:
        _HANDLES[key] = engine("go1gate", N, **kw)
    return _HANDLES[key]


def synth(name, N, T, L, seed=0):
    key = (name, N, T, L, seed)
    if key not in _SYNTH:
        _SYNTH[key] = ref.synth(name, N, T, L, D=D, seed=seed)
    return _SYNTH[key]


def install(eng, s, value_norm=False):
    eng.create_actor(s["a_dims"], s["c_dims"], activation=s["act"], layer_norm=s["hidden"], feature_norm=s["feat"], recurrent=True, value_norm=value_norm)
    views = eng.actor_params()
    views["flat"].copy_(gru_ref.flat_params(*s["nets"]))
    assert views["flat"].numel() == s["n_params"] and tuple(eng.tensor(abi.T_WRAPPER_OBS).shape) == (s["N"], s["Aw"], s["D"])
    assert eng.rollout_row_stride() == s["p4"] and eng.hidden_width() == s["Hs"]
    return views


def upload(s, dev, ret=None):
    t = {k: torch.from_numpy(s[k].copy()).to(dev) for k in ("packed", "value", "grad", "stats")}
    t.update({k: s[k].to(dev).contiguous() for k in ("actions", "logp_old", "adv", "index")})
    t["ret"] = (s["ret"] if ret is None else ret).to(dev).contiguous()
    return t


def call(eng, s, t, L, first, count, use_index, cfg=ref.CFG, flags=None, **kw):
    loss = abi.PpoLoss(cfg["clip"], cfg["value_coef"], cfg["entropy_coef"], cfg["value_clip"] if cfg["value_clip"] is not None else 0.0)
    a = dict(T=s["T"], packed=t["packed"].data_ptr(), stride=s["stride"], index=t["index"].data_ptr() if use_index else None, first=first, count=count,
             flags=(abi.PPO_CLIP_VALUE if cfg["value_clip"] is not None else 0) | abi.PPO_BPTT | L << abi.PPO_CHUNK_SHIFT if flags is None else flags,
             stats=t["stats"].data_ptr())
    a.update(kw)
    rc = eng.lib.mqe_ppo_grad(eng.h, a["T"], a["packed"], a["stride"], t["actions"].data_ptr(), t["logp_old"].data_ptr(), t["value"].data_ptr(), t["adv"].data_ptr(),
                              t["ret"].data_ptr(), a["index"], a["first"], a["count"], C.byref(loss), a["flags"], t["grad"].data_ptr(), a["stats"], eng._stream())
    torch.cuda.synchronize()
    return rc


def outputs(s, t):
    return t["grad"][:s["n_params"]].view(torch.float32).cpu(), t["stats"][:6].view(torch.float32).cpu()


selection = ref.selection


def check(s, t, chunks, L, cfg, what, src=None):
    """the kernel's gradient and statistics of the minibatch `chunks` against the float64 twin; src: the trajectory the reference reads (value
    normalisation: the one whose `ret` holds the normalised targets)"""
    src = src or s
    grad, stats = outputs(s, t)
    g64, st64, S = ref.manual(src, chunks, L, cfg)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(stats).all()), what
    got = {n: grad[o:o + int(np.prod(shp))].reshape(shp).numpy() for n, (o, shp) in
           abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True).items()}
    worst, at = ref.ratio_to_bound(got, g64, S)
    # the statistics (the module docstring)
    with torch.no_grad():
        a32, c32, ls = src["nets"]
        a64, c64 = gru_ref.doubles(a32, c32)
        m64, v64 = ref.twin_outputs(a64, c64, src, chunks, L, torch.float64)
        m32, v32 = ref.twin_outputs(a32, c32, src, chunks, L, torch.float32)
    b = ref.sample_data(src, chunks, L)
    logp = lambda m: ((-0.5 * ((b["actions"] - m.double()) * torch.exp(-ls.double())) ** 2 - ls.double()).sum(-1) - 1.5 * ref.LN2PI)
    e_p = 4 * float((logp(m32) - logp(m64)).abs().max()) + 2.0 ** -22
    e_v = 4 * float((v32.double() - v64).abs().max()) + 2.0 ** -22
    ratio = torch.exp(logp(m64) - b["logp_old"])
    d = torch.maximum((v64 - b["ret"]).abs(), (b["v_old"] - b["ret"]).abs() + (cfg["value_clip"] or 0.0))
    tol = [float((b["adv"].abs() * ratio).mean()) * math.expm1(e_p), float((2 * d + e_v).mean()) * e_v, 0.0, 0.0, e_p, 0.0]
    tol[3] = tol[0] + cfg["value_coef"] * tol[1]
    tol = [x + 2.0 ** -22 * (1 + abs(float(st64[i]))) for i, x in enumerate(tol)]
    dev = np.abs(stats.double().numpy() - st64)
    print(f"bptt_kernel {what}: gradient {worst:.2f} x 2^-24 S at {at} (bound {ref.K_GPU:.0f}); statistics / their bounds " +
          " ".join(f"{x / y:.2f}" for x, y in zip(dev[:5], tol[:5])))
    assert worst <= ref.K_GPU, (what, worst, at)
    assert stats[5].item() == np.float32(st64[5]), "kink-free inputs: the same clip count"
    assert all(dev[i] <= tol[i] for i in range(5)), (what, dev, tol)


def run(group, name, engine_n=None):
    """the calls of bptt_ref.CASES[group] for the shape `name`: the minibatches K_CPU was measured on"""
    for nm, N, T, L, calls in ref.CASES[group]:
        if nm != name:
            continue
        s = synth(nm, N, T, L)
        if L >= 2:
            inside, at0 = ref.resets_inside(s, np.arange(s["n_chunks"]), L)
            assert inside >= 0.25 and at0 > 0, "at least a quarter of the chunks hold a reset inside, some at their first step"
        eng = handle(N)
        install(eng, s)
        for first, count, use_index, vclip in calls:
            cfg = dict(ref.CFG, value_clip=ref.VALUE_CLIP if vclip else None)
            t = upload(s, eng.torch_device)
            rc = call(eng, s, t, L, first, count, use_index, cfg)
            assert rc == 0, eng.lib.mqe_last_error().decode()
            check(s, t, selection(s, first, count, use_index), L, cfg, f"{nm} L={L} chunks={count} first={first} index={use_index} vclip={vclip}")


# ---- 1. the gradient against float64 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_gradient_against_float64_over_shapes(name):
    """every shape of bptt_ref.SHAPES -- cells 5 / 7 (dword loads), 16 / 12, 64 / 48 and 64 / 64 wide, two and three Linear layers, tanh and relu,
    plain, hidden norm, feature norm, both -- at L = 5 on N = 4, T = 10 (16 chunks): all chunks by an index list, a range with first > 0, and a call
    without value clipping.  tanh64x64_both takes 32-chunk tiles by the LDS rule, tanh64_48 64-chunk tiles."""
    a_dims, c_dims, _, hidden, feat = ref.dims_of(name, D)
    want_rt = {"tanh64x64_both": 32, "tanh64_48": 64}.get(name)
    if want_rt:
        assert abi.bptt_row_tile(a_dims, c_dims, hidden, feat) == want_rt
    run("shapes", name)


@pytest.mark.parametrize("name", ["tanh7_5", "tanh64x64_both"])
def test_chunk_lengths(name):
    """L = 1 (no carried gradient), L = 2, and L = T = 10 (one chunk per row); L = 5 is the test above"""
    run("lengths", name)


@pytest.mark.parametrize("name", ["tanh7_5", "tanh64_48", "tanh64x64_both"])
def test_chunk_counts_at_the_tile_edges(name):
    """1, 63, 64, 65 and 130 chunks of L = 2 (N = 4, T = 34: 136 chunks): the edges of a 64-chunk tile, and of two and four 32-chunk tiles"""
    run("counts", name)


# ---- 2. more tiles than workgroups ----------------------------------------------------------------------------------------------------------------------------
def test_a_workgroup_walks_a_second_tile():
    """18 432 chunks (N = 1024, T = 18, L = 2) are 288 tiles of 64 for 256 workgroups: the partial gradients continue their chains through the
    scratch, `first` holds on a workgroup's first tile and last step only.  The smallest networks."""
    a_dims, c_dims, _, hidden, feat = ref.dims_of("tanh7_5", D)
    assert abi.bptt_row_tile(a_dims, c_dims) == 64 and 18432 > 256 * 64
    run("tiles", "tanh7_5")


# ---- 3. value normalisation -----------------------------------------------------------------------------------------------------------------------------------
def test_value_normalisation_with_update():
    """MQE_PPO_VALUE_NORM | _UPDATE: k_bptt_expand's list feeds k_vn_moments / k_vn_apply, so the state is updated from the count L returns of the
    minibatch's chunks and the loss reads them normalised at their own positions.  The reference reads the targets the kernels store
    (value_norm_ref.normalise32 with the updated state) as data"""
    L = 5
    s = synth("tanh9x5_6x7_both", 4, 10, L)
    eng = handle(4)
    views = install(eng, s, value_norm=True)
    state = vnref.k_state()
    views["value_norm"].copy_(torch.from_numpy(state))
    raw = (s["ret"].double() * float(state[4]) + float(state[3])).float()           # returns in reward units whose normalised values are the kink-free targets
    first, count = 3, 11
    chunks = selection(s, first, count, True)
    tt, r = ref.chunk_steps(s, chunks, L)
    x = raw[tt, r[None, :]]
    t = upload(s, eng.torch_device, ret=raw)
    rc = call(eng, s, t, L, first, count, True, flags=abi.PPO_CLIP_VALUE | abi.PPO_VALUE_NORM | abi.PPO_VALUE_NORM_UPDATE | abi.PPO_BPTT | L << abi.PPO_CHUNK_SHIFT)
    assert rc == 0, eng.lib.mqe_last_error().decode()
    after = views["value_norm"].cpu().numpy().copy()
    want = vnref.update(state, x.numpy())
    for got, w, tol in zip(after[:3], want, vnref.tol_update(state, x.numpy())):
        assert abs(float(got) - float(w)) <= tol, "the statistics fold in the returns of the chunks' count L samples"
    src = dict(s, ret=s["ret"].clone())
    src["ret"][tt, r[None, :]] = torch.as_tensor(np.asarray(vnref.normalise32(x.numpy(), after[3], after[4]), dtype=np.float32))
    check(s, t, chunks, L, ref.CFG, "value_norm + update tanh9x5_6x7_both L=5", src=src)
    assert same_bits(t["ret"].cpu(), raw), "the caller's returns stay as they are"


# ---- 3a. chunk numbers outside the trajectory ------------------------------------------------------------------------------------------------------------------
def clamped_selection():
    """the smallest recurrent shape (16 chunks of L = 5, one tile) with an index list that holds numbers below 0, numbers past the last chunk and one chunk
    twice -> (s with that list, L, first, count, the chunks the kernels must read: the list clipped into [0, n_chunks)).  synth() makes every chunk
    kink-free on its own, so a selection out of existing chunks is kink-free too: held here with the float64 twin, at synth()'s own margins"""
    L = 5
    s = synth("tanh9x5_6x7_both", 4, 10, L)
    s = dict(s, index=torch.tensor([7, -3, 5, 16, 5, 1000, 2, 15, -2 ** 31, 2 ** 31 - 1, 9, 11], dtype=torch.int32))
    first, count = 1, 10
    chunks = np.clip(s["index"][first:first + count].numpy().astype(np.int64), 0, s["n_chunks"] - 1)
    assert chunks.min() == 0 and chunks.max() == s["n_chunks"] - 1 and len(set(chunks.tolist())) < count
    a64, c64 = gru_ref.doubles(*s["nets"][:2])
    kinked = ref._kinked(s, (a64, c64, s["nets"][2]), chunks, L, dict(clip=ref.CLIP, value_clip=ref.VALUE_CLIP))[0]
    assert not bool(kinked.any()), "the clipped selection keeps every sample the kink margin away from the loss's kinks"
    return s, L, first, count, chunks


def test_chunk_numbers_outside_the_trajectory_are_clamped():
    """a chunk number outside [0, (T / L) R') is the caller's error and the kernel clamps it (bptt_chunks): the gradient and the statistics are those of
    the clipped list, a duplicate counted twice"""
    s, L, first, count, chunks = clamped_selection()
    eng = handle(4)
    install(eng, s)
    t = upload(s, eng.torch_device)
    rc = call(eng, s, t, L, first, count, True)
    assert rc == 0, eng.lib.mqe_last_error().decode()
    check(s, t, chunks, L, ref.CFG, f"clamped chunk numbers tanh9x5_6x7_both L={L} chunks={count}")
    assert torch.equal(t["index"].cpu(), s["index"]), "the list is read only"


def test_clamped_chunk_numbers_under_value_normalisation_with_update():
    """the same selection under MQE_PPO_VALUE_NORM | _UPDATE (k_bptt_expand clamps, k_vn_moments / k_vn_apply read its list): the statistics fold in the
    returns of the clipped chunks' count L samples, a duplicated chunk's as often as it occurs, and the loss reads them normalised"""
    s, L, first, count, chunks = clamped_selection()
    eng = handle(4)
    views = install(eng, s, value_norm=True)
    state = vnref.k_state()
    views["value_norm"].copy_(torch.from_numpy(state))
    raw = (s["ret"].double() * float(state[4]) + float(state[3])).float()
    tt, r = ref.chunk_steps(s, chunks, L)
    x = raw[tt, r[None, :]]
    assert x.numel() == count * L
    t = upload(s, eng.torch_device, ret=raw)
    rc = call(eng, s, t, L, first, count, True, flags=abi.PPO_CLIP_VALUE | abi.PPO_VALUE_NORM | abi.PPO_VALUE_NORM_UPDATE | abi.PPO_BPTT | L << abi.PPO_CHUNK_SHIFT)
    assert rc == 0, eng.lib.mqe_last_error().decode()
    after = views["value_norm"].cpu().numpy().copy()
    want = vnref.update(state, x.numpy())
    for got, w, tol in zip(after[:3], want, vnref.tol_update(state, x.numpy())):
        assert abs(float(got) - float(w)) <= tol, "the statistics fold in the returns of the clipped chunks' count L samples"
    src = dict(s, ret=s["ret"].clone())
    src["ret"][tt, r[None, :]] = torch.as_tensor(np.asarray(vnref.normalise32(x.numpy(), after[3], after[4]), dtype=np.float32))
    check(s, t, chunks, L, ref.CFG, "clamped chunk numbers, value_norm + update tanh9x5_6x7_both L=5", src=src)
    assert same_bits(t["ret"].cpu(), raw), "the caller's returns stay as they are"


# ---- 4. determinism, coverage, refusals -------------------------------------------------------------------------------------------------------------------------
def test_same_bits_full_write_and_refusals():
    L = 5
    s = synth("tanh9x5_6x7_both", 4, 10, L)
    eng = handle(4)
    install(eng, s)
    dev = eng.torch_device
    a, b = upload(s, dev), upload(s, dev)
    assert call(eng, s, a, L, 0, 16, True) == 0 and call(eng, s, b, L, 0, 16, True) == 0
    assert same_bits(a["grad"], b["grad"]) and same_bits(a["stats"], b["stats"]), "two identical calls give the same bits"
    sent = lambda x: x.view(torch.int32) == ref.SENT
    assert not bool(sent(a["grad"][:s["n_params"]]).any()) and bool(sent(a["grad"][s["n_params"]:]).all()), "grad_dev is written in full, nothing beyond"
    assert not bool(sent(a["stats"][:6]).any()) and bool(sent(a["stats"][6:]).all())
    assert torch.equal(a["packed"].cpu(), torch.from_numpy(s["packed"])), "the trajectory is read only"

    def refused(word, **kw):
        t = upload(s, dev)
        rc = call(eng, s, t, kw.pop("L", L), kw.pop("first", 0), kw.pop("count", 4), kw.pop("use_index", False), **kw)
        msg = eng.lib.mqe_last_error().decode()
        assert rc == -6 and word in msg, (rc, msg, word)
        assert bool(sent(t["grad"]).all()) and bool(sent(t["stats"]).all()), "a refused call writes nothing"
        return msg
    bptt = abi.PPO_BPTT
    assert "1 .. MQE_PPO_MAX_CHUNK" in refused("flags", flags=bptt)                                         # L = 0
    assert "1 .. MQE_PPO_MAX_CHUNK" in refused("flags", flags=bptt | 65 << abi.PPO_CHUNK_SHIFT)
    refused("T must be a multiple", flags=bptt | 3 << abi.PPO_CHUNK_SHIFT)
    refused("row_stride", stride=s["p4"])
    refused("row_stride", stride=s["p4"] + s["R"] * s["Hs"] - 4)
    refused("chunks", first=10, count=7)                                                                    # 16 chunks
    assert "back-propagation through time" in refused("MQE_PPO_BPTT", flags=0)                             # a recurrent handle without the bit
    assert "back-propagation through time" in refused("MQE_PPO_BPTT", flags=5 << abi.PPO_CHUNK_SHIFT)
    # a plain handle: the bit, or a length alone
    eng.create_actor([D, 7, 3], [D, 5, 1])
    for fl in (bptt | L << abi.PPO_CHUNK_SHIFT, bptt, 1 << abi.PPO_CHUNK_SHIFT, 0x80 << abi.PPO_CHUNK_SHIFT):
        assert "MQE_ACTOR_RECURRENT" in refused("flags", flags=fl)


# ---- 5. a real rollout -----------------------------------------------------------------------------------------------------------------------------------------
def _recorded(name, seed):
    eng = engine("go1gate", 6, seed=seed, max_episode_length=5)
    a_dims, c_dims, act, hidden, feat = ref.dims_of(name, D)
    actor, critic, log_std = gru_ref.make_nets(D, tuple(a_dims[1:-1]), tuple(c_dims[1:-1]), act, hidden, feat, seed=9)
    eng.create_actor(a_dims, c_dims, activation=act, layer_norm=hidden, feature_norm=feat, recurrent=True)
    eng.actor_params()["flat"].copy_(gru_ref.flat_params(actor, critic, log_std))
    eng.reset_all()
    eng.rollout(3)                                     # not from a fresh state: row 0's tail is non-zero
    traj = eng.rollout(10, record_hidden=True, time_outs=True)
    eng.gae(traj, 0.99)
    torch.cuda.synchronize()
    return eng, traj, (actor, critic, log_std), dict(a_dims=a_dims, c_dims=c_dims, act=act, hidden=hidden, feat=feat)


def _as_synth(traj, nets, shape, N, L):
    """the logical tensors of a recorded trajectory in bptt_ref's form (host copies)"""
    T, R = int(traj.T), N * 2
    s = dict(shape, N=N, Aw=2, T=T, D=D, R=R, L=L, n_chunks=(T // L) * R, nets=nets, Hs=traj.hidden.shape[-1])
    s["obs"] = traj.obs.cpu().reshape(T + 1, R, D)
    s["done"] = torch.cat([torch.zeros(1, N, dtype=torch.uint8), traj.done.cpu().to(torch.uint8)])       # row 0's done bytes are zero
    s["tails"] = traj.hidden.cpu().reshape(T + 1, R, -1)
    s["actions"], s["logp_old"], s["adv"] = traj.actions.cpu().reshape(T, R, 3), traj.logp.cpu().reshape(T, R), traj.advantages.cpu().reshape(T, R)
    s["v_old"], s["ret"] = traj.value.cpu()[:T].reshape(T, R), traj.returns.cpu().reshape(T, R)
    s["params"] = ref.named(*nets, shape["a_dims"], shape["c_dims"], shape["hidden"], shape["feat"])
    s["n_params"] = abi.actor_param_count(shape["a_dims"], shape["c_dims"], False, shape["hidden"], shape["feat"], recurrent=True)
    return s


@pytest.mark.parametrize("name", ["tanh9x5_6x7_both", "tanh7_5"])
def test_real_rollout_unchanged_parameters(name):
    """rollout(T = 10, record_hidden=True) with max_episode_length = 5, then ppo_grad(chunk_length = L) with the parameters that rolled out: logp is
    logp_old up to the forward's rounding, so the clip share is exactly 0 and the approximate KL is the float64 twin's mean(logp_old - logp64) within
    4 x the float32 twin's largest per-sample deviation (gru_ref's yardstick).  Holds the chunk, tail and done addressing to what mqe_rollout wrote"""
    N = 6
    eng, traj, nets, shape = _recorded(name, seed=21)
    assert bool(traj.done.any()) and float(traj.hidden[0].abs().max()) > 0
    a64, c64 = gru_ref.doubles(nets[0], nets[1])
    for L in (1, 5, 10):
        grad, stats = eng.ppo_grad(traj, chunk_length=L, value_clip=0.2)
        torch.cuda.synchronize()
        s = _as_synth(traj, nets, shape, N, L)
        chunks = np.arange(s["n_chunks"])
        _, st64, lp64 = ref.autograd(s, chunks, L, dict(ref.CFG, value_coef=1.0, entropy_coef=0.0))
        _, _, lp32 = ref.autograd(s, chunks, L, dict(ref.CFG, value_coef=1.0, entropy_coef=0.0), torch.float32)
        yard = float((lp32.double() - lp64).abs().max())
        kl = float(stats[4])
        print(f"bptt_rollout {name} L={L}: KL {kl:.3e} float64 {float(st64[4]):.3e} yardstick {yard:.3e} clip share {float(stats[5])}")
        assert float(stats[5]) == 0.0
        assert abs(kl - float(st64[4])) <= 4 * yard + 2.0 ** -24
        assert bool(torch.isfinite(grad).all())
    with pytest.raises(ValueError, match="not a multiple"):
        eng.ppo_grad(traj, chunk_length=3)
    plain = eng.rollout(10)
    eng.gae(plain, 0.99)
    with pytest.raises(ValueError, match="traj.hidden is None"):
        eng.ppo_grad(plain, chunk_length=5)
    eng.close()


def test_real_rollout_ppo_update_against_the_float64_twin():
    """one ppo_update(epochs=1, minibatches=2, chunk_length=5) with a seeded generator: the parameters lie within ppo_ref.adam_tolerances (+ the
    gradient's own bound through Adam's step) of the float64 twin trained on the same permutation; the cells and gru.norm.* have moved"""
    N, L, name = 6, 5, "tanh9x5_6x7_both"
    eng, traj, nets, shape = _recorded(name, seed=22)
    dev = eng.torch_device
    views = eng.actor_params()
    before = views["flat"].cpu().clone()
    s = _as_synth(traj, nets, shape, N, L)
    gen = torch.Generator(device=dev).manual_seed(5)
    perm = torch.randperm(s["n_chunks"], device=dev, generator=torch.Generator(device=dev).manual_seed(5)).cpu().numpy()
    lr, cfg = 1e-3, dict(clip=0.2, value_coef=1.0, entropy_coef=0.0, value_clip=None)
    stats = eng.ppo_update(traj, epochs=1, minibatches=2, lr=lr, chunk_length=L, generator=gen)
    torch.cuda.synchronize()
    after = views["flat"].cpu().clone()
    assert stats.shape == (1, 2, 6) and eng.ppo_step == 2
    # the float64 twin on the same two minibatches
    p = before.double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    tol, tol_adam = torch.zeros_like(p), torch.zeros_like(p)
    per = s["n_chunks"] // 2
    for b in range(2):
        chunks = perm[b * per:(b + 1) * per] if b == 0 else perm[per:]
        sb = dict(s, params={k: t.double() for k, t in ppo_ref_split(p, s).items()})
        g64, _, S = ref.manual(sb, chunks, L, cfg)
        g = ref.flat_of(g64, s)
        gb = ref.flat_of({k: np.full_like(np.asarray(g64[k], dtype=np.float64), S[k]) for k in g64}, s) * (ref.K_GPU * ref.EPS32)
        tp, _, _ = ppo_ref.adam_tolerances(p.float(), m.float(), v.float(), g.float(), b + 1, lr)
        # a gradient error dg moves Adam's update by at most step_size dg / (sqrt(v) / bc2s + eps) <= lr dg / |g| at the first steps; bounded by lr
        tol = tol + tp + lr * torch.minimum(gb / g.abs().clamp_min(1e-30), torch.ones_like(g)) * 2
        tol_adam = tol_adam + tp
        p, m, v, _ = ppo_ref.adam(p, m, v, g, b + 1, lr)
    dev_p = (after.double() - p).abs()
    print(f"bptt_update: worst parameter deviation {float((dev_p / tol.clamp_min(1e-30)).max()):.3f} of its tolerance; of adam_tolerances alone "
          f"{float((dev_p / tol_adam.clamp_min(1e-30)).max()):.3f}")
    assert bool((dev_p <= tol).all())
    lay = abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True)
    for n_, (o, shp) in lay.items():
        if ".gru." in n_:
            k = int(np.prod(shp))
            assert float((after[o:o + k] - before[o:o + k]).abs().max()) > 0, f"{n_} has moved"
    eng.close()


def ppo_ref_split(flat, s):
    lay = abi.actor_param_layout(s["a_dims"], s["c_dims"], False, s["hidden"], s["feat"], recurrent=True)
    return {n: flat[o:o + int(np.prod(shp))].reshape(shp) for n, (o, shp) in lay.items()}
