"""Host side of the GAE tests (mqe_gae, csrc/kernels_gae.hpp): the recursion restated in numpy -- float64 as the reference, float32 with
the kernel's roundings as its twin, and deliberately wrong variants -- the derived tolerances, and the seeded synthetic trajectory in
mqe_rollout's layout that the CPU and the GPU tests share."""
import numpy as np

EPS32 = 2.0 ** -24
SENT = 0x7FC12345          # the sentinel of tests/test_rollout_gpu.py: a NaN pattern none of whose bytes is 0 or 1

SHAPES = [(1, 2, 1), (3, 2, 5), (5, 2, 12), (33, 2, 7), (64, 2, 9), (2, 2, 300), (3, 2, 16)]      # (N, A', T); 16 = two full batches of 8
GAMMA_LAM = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)]


def _fma32(a, b, c):
    """fmaf: the product of two float32 is exact in float64; one rounding of the sum to float32"""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def gae(reward, value, done, time_outs, gamma, lam, dtype=np.float64, variant=None):
    """reward (T, N, A), value (T+1, N, A), done (T, N) 0/1, time_outs (T, N) bytes or None -> (adv, ret) (T, N, A) of `dtype`.
    float64: plain arithmetic.  float32: the kernel's statement -- fmaf where it has one, gamma * lam one float32 product.
    variant "timeout_is_failure": the time-out bootstrap left out; "vn_unmasked": gamma * value[t + 1] added at a done as well."""
    T = reward.shape[0]
    f32 = dtype == np.float32
    g = dtype(gamma)
    gl = dtype(np.float32(gamma) * np.float32(lam)) if f32 else g * dtype(lam)
    fma = _fma32 if f32 else (lambda a, b, c: a * b + c)
    r, v = reward.astype(dtype), value.astype(dtype)
    adv = np.zeros(reward.shape, dtype)
    ret = np.zeros(reward.shape, dtype)
    run = np.zeros(reward.shape[1:], dtype)
    for t in range(T - 1, -1, -1):
        d = (done[t] != 0)[:, None]
        to = ((time_outs[t] & done[t]) != 0)[:, None] if time_outs is not None and variant != "timeout_is_failure" else np.zeros_like(d)
        rr = np.where(to, fma(g, v[t], r[t]), r[t])
        boot = fma(g, v[t + 1], rr)
        delta = (boot if variant == "vn_unmasked" else np.where(d, rr, boot)) - v[t]
        run = np.where(d, delta, fma(gl, run, delta)).astype(dtype)
        adv[t] = run
        ret[t] = run + v[t]
    return adv, ret


def tolerances(reward, value, adv64, gamma, lam):
    """(tol_adv, tol_ret), derived: a step has four float32 roundings -- rr, the inner fmaf, the subtraction, the fmaf into adv -- each at most
    2^-24 times the magnitude it rounds, and B = max over (t, r) of |reward| + 2 gamma |v| + gamma |vn| + |v| + gamma lam |adv64[t+1]| +
    |adv64[t]| bounds every one of them; an error made at step t reaches step t - k scaled by (gamma lam)^k:
    tol_adv = 4 2^-24 B sum_{k<T} (gamma lam)^k;  ret = adv + v is one more rounding: tol_ret = tol_adv + 2^-24 max(|adv64| + |v|)."""
    T = reward.shape[0]
    r, v = np.abs(reward.astype(np.float64)), np.abs(value.astype(np.float64))
    a = np.abs(adv64)
    a_next = np.concatenate([a[1:], np.zeros_like(a[:1])])
    B = float((r + 2 * gamma * v[:-1] + gamma * v[1:] + v[:-1] + gamma * lam * a_next + a).max())
    tol_adv = 4 * EPS32 * B * float(sum((gamma * lam) ** k for k in range(T)))
    return tol_adv, tol_adv + EPS32 * float((a + v[:-1]).max())


def synth(N, Aw, T, D, seed, extra_stride=8, guard=64):
    """A seeded trajectory that hits every branch of the recursion, in mqe_gae's buffers: rewards U(-1, 1), values 2 N(0, 1), done with
    p = 0.15 per (t, env), a time-out on about half of the dones, time-out bytes set on about a tenth of the steps that are NOT done
    (must be ignored), env 0 done at t = 0 (a time-out) and at t = T - 1 (T >= 2: a failure), the last env never done (N >= 2).
    -> dict: reward, value, done, time_outs (numpy, logical shapes) and the flat int32 images `packed` ((T + 1) * stride + guard words:
    reward floats and done bytes of rows 1 .. T in place, everything else the sentinel), `adv` / `ret` / `stats` (sentinel, guard behind)."""
    rng = np.random.default_rng(seed)
    R = N * Aw
    reward = rng.uniform(-1, 1, (T, N, Aw)).astype(np.float32)
    value = (2 * rng.standard_normal((T + 1, N, Aw))).astype(np.float32)
    done = (rng.random((T, N)) < 0.15).astype(np.uint8)
    done[0, 0] = 1
    if T >= 2:
        done[T - 1, 0] = 1
    if N >= 2:
        done[:, N - 1] = 0
    time_outs = (done & (rng.random((T, N)) < 0.5)).astype(np.uint8)
    time_outs[0, 0] = 1
    if T >= 2:
        time_outs[T - 1, 0] = 0
    stray = (done == 0) & (rng.random((T, N)) < 0.1)
    free = np.argwhere(done == 0)
    if len(free):
        stray[tuple(free[0])] = True          # at least one wherever a step that is not done exists
    time_outs[stray] = 1
    nobs = R * D
    pf = nobs + R + (N + 3) // 4
    stride = (pf + 3) // 4 * 4 + extra_stride
    packed = np.full((T + 1) * stride + guard, SENT, np.int32)
    rows = packed[:(T + 1) * stride].reshape(T + 1, stride)
    rows[1:, nobs:nobs + R] = reward.reshape(T, R).view(np.int32)
    tail = rows[1:, nobs + R:pf].copy().view(np.uint8).reshape(T, -1)
    tail[:, :N] = done
    rows[1:, nobs + R:pf] = tail.view(np.int32).reshape(T, -1)
    out = lambda n: np.full(n + guard, SENT, np.int32)
    return dict(N=N, Aw=Aw, T=T, D=D, R=R, nobs=nobs, pf=pf, stride=stride, guard=guard, reward=reward, value=value, done=done,
                time_outs=time_outs, stray=stray, packed=packed, adv=out(T * R), ret=out(T * R), stats=out(2))
