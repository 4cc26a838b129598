"""CPU self-test of the step-wise bf16 verifier (oracle/bf16_stepwise.py): it must accept the state a
correct bf16 path leaves behind and reject five seeded defects, so the GPU tests built on it
(tests/test_gpu_bf16_blocks.py) are neither vacuous nor over-tight.

The "GPU state" here is oracle.lstm_bf16.gpu_state: the bf16-mode oracle on torch fp32 ops (another
summation order than the verifier's fp64), in the HIP path's layouts.  The tie-near cap (<= 2 % of
the x-projection elements within 2^-21 of the absolute sum of a bf16 rounding tie) is asserted here,
from the reference alone, for every parametrised input of the GPU tests (bf16_cases)."""
import functools

import pytest
import torch

import bf16_cases
from oracle import bf16_stepwise as sw
from oracle import lstm_bf16

SHAPES = [(7, 8, 40, 2, 3), (9, 16, 72, 2, 4), (65, 40, 96, 3, 3)]   # (B, F, H, L, T)


@functools.lru_cache(maxsize=None)
def _clean(B, F, H, L, T):
    sd, x, demb = bf16_cases.inputs(B, F, H, L, T, bf16_cases.P_SMALL)
    return lstm_bf16.gpu_state(sd, x, demb, L)


def _verify(name, shape, st, fused):
    """The whole verifier over a proxy state; fused: the x-projection taken as unreadable."""
    B, F, H, L, T = shape
    sd, _, demb = bf16_cases.inputs(B, F, H, L, T, bf16_cases.P_SMALL)
    ws, w_p, b_p = bf16_cases.layer_weights(sd, L)
    rep = sw.Report(name)
    sw.verify_forward(rep, ws, st, xp_gpu=None if fused else st["xp"])
    top = [torch.zeros(T, B, H, dtype=dt) for dt in (sw.F64, sw.F32)]
    for a, dt in zip(top, (sw.F64, sw.F32)):
        a[T - 1] = sw.proj_backward(st["h_tm"][L - 1][T], w_p, b_p, demb, dt)
    grads = {(l, k): st["grads"][f"LSTM_stack.{n}_l{l}"] for l in range(L)
             for k, n in (("w_ih", "weight_ih"), ("w_hh", "weight_hh"), ("b_ih", "bias_ih"), ("b_hh", "bias_hh"))}
    sw.verify_backward(rep, ws, st, top, grads=grads, dx={l: st["dx"][l] for l in range(L)})
    return rep


def test_q64_is_rne_to_bf16():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(4096, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g)
    v32 = v.to(torch.float32)  # exactly representable in fp32: torch's fp32 -> bf16 cast is one RNE rounding
    assert torch.equal(sw.q64(v32.double()), v32.to(torch.bfloat16).double())
    ties = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(2.0 + 2.0 ** -7)], dtype=torch.float64)
    assert torch.equal(sw.q64(ties), torch.tensor([1.0, 1.0 + 2.0 ** -6, -2.0], dtype=torch.float64))
    assert torch.equal(sw.tie_distance(ties), torch.zeros(3, dtype=torch.float64))
    assert float(sw.tie_distance(torch.tensor([1.0], dtype=torch.float64))) == 2.0 ** -8
    assert float(sw.ulp_bf16(torch.tensor([1.5], dtype=torch.float64))) == 2.0 ** -7


@pytest.mark.parametrize("case", bf16_cases.all_stack_inputs(), ids=lambda c: "B{}F{}H{}L{}T{}".format(*c[:5]))
def test_tie_near_cap_of_every_gpu_test_input(case):
    """Every layer's x-projection of every input the GPU tests use: tie-near share <= 2 %, from the
    reference alone (layer l > 0 from the bf16 oracle's h of the layer below)."""
    B, F, H, L, T, P = case
    sd, x, _ = bf16_cases.inputs(*case)
    ws, _, _ = bf16_cases.layer_weights(sd, L)
    _, (caches, _, _, _) = lstm_bf16.embedder_forward(sd, x, L)
    rep = sw.Report("tie.B{}F{}H{}L{}T{}".format(*case[:5]))
    for l in range(L):
        inp = caches[l][0].transpose(0, 1).double()   # q(input) [T,B,F_l]
        sw.x_projection(rep, f"l{l}.xp", inp, ws[l][0], ws[l][2], ws[l][3])
    assert rep.tie_share <= sw.TIE_CAP


@pytest.mark.parametrize("fused", [False, True], ids=["xp_read", "xp_fused"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B{}F{}H{}L{}T{}".format(*s))
def test_verifier_accepts_the_oracle_state(shape, fused):
    rep = _verify("accept", shape, _clean(*shape), fused)
    print(f"\nMEASURED verifier.accept worst of-bound {rep.worst:.3f} at {rep.worst_at}; tie-near {rep.tie_share:.2e}")
    assert 0.0 < rep.worst <= 1.0


def _defect_state(defect, shape):
    B, F, H, L, T = shape
    sd, x, demb = bf16_cases.inputs(B, F, H, L, T, bf16_cases.P_SMALL)
    clean = _clean(*shape)

    def tap(name, l, t, v):
        if defect == "c_t_for_c_prev" and name == "c_prev_bwd":
            return clean["c_tm"][l][t]                      # c_t in the forget gate's gradient
        if defect == "k_tail_dropped" and name == "hq":
            v = v.clone()
            v[:, H - 8:] = 0                                # the last 8 columns of K = H
            return v
        if defect == "c_prev_row_above" and name == "c_prev" and t > 0 and l == L - 1:
            v = v.clone()
            v[B - 1] = v[B - 2]                             # one row tail's c_prev
            return v
        if defect == "o_gate_scaled" and name == "z":
            v = v.clone()
            v[:, 3 * H:] *= 1.0 + 2.0 ** -10
            return v
        return v

    st = lstm_bf16.gpu_state(sd, x, demb, L, tap=tap)
    if defect == "hT_padding":
        st["hT"][0].view(H, T + 1, st["Bp"])[:, 1, B:] = 1.0
    return st


DEFECTS = ["c_t_for_c_prev", "k_tail_dropped", "c_prev_row_above", "hT_padding", "o_gate_scaled"]


@pytest.mark.parametrize("fused", [False, True], ids=["xp_read", "xp_fused"])
@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "B{}F{}H{}L{}T{}".format(*s))
def test_verifier_rejects_seeded_defect(shape, defect, fused):
    """Each defect seeded into the proxy's step is rejected -- also o_gate_scaled (the o gate's
    pre-activation times 1 + 2^-10), which no end-to-end bf16 tolerance of the suite sees."""
    st = _defect_state(defect, shape)
    with pytest.raises(sw.Mismatch) as e:
        _verify(f"reject.{defect}", shape, st, fused)
    print(f"\nMEASURED verifier.reject {defect}: {e.value}")
