"""The parametrised inputs of the bf16 step-wise tests, shared by tests/test_gpu_bf16_blocks.py (the
HIP kernels) and tests/test_bf16_stepwise_verifier.py (the verifier's CPU self-test, which also
asserts the tie-near cap of oracle/bf16_stepwise.py for every one of these inputs before any GPU
time is spent).  Seeds are fixed here; recipe.make_weights at scale 3 as everywhere in the suite."""
import functools

import numpy as np

import recipe

# (B, F, H, T): one layer through the C ABI
LAYER_CASES = [(1, 8, 8, 1),       # a single partial tile, T = 1
               (7, 8, 40, 3),      # partial row, unit and k tiles, Bp padding
               (64, 40, 32, 2),    # the exact 64 x 32 tile, Bp == B
               (65, 40, 96, 3),    # a second row block of one row, k tail of 32
               (9, 16, 72, 4)]     # unit tail of 8, k tail of 8
# (B, F, H, L, T): the stack under per_step and persist
STACK_CASES = [(35, 8, 64, 2, 3), (64, 40, 64, 3, 2), (65, 40, 96, 3, 4), (64, 8, 96, 2, 3)]
# (B, T, schedule) at F = 40, H = 768, L = 3 (tests/test_gpu_bf16_blocks.py says which kernel each reaches)
H768_CASES = [(33, 4, "auto"), (80, 3, "auto"), (84, 3, "per_layer"), (160, 3, "per_layer"),
              (288, 3, "per_layer"), (340, 3, "per_layer")]
P_SMALL, P_768 = 16, 256
# seeds moved where the first draw broke the verifier's tie-near cap (computed on the CPU from the
# reference alone): at B = 1, H = 8, T = 1 the x-projection has 32 elements, so one tie-near element
# is 3.1 % > 2 %
SEED_SHIFT = {(1, 8, 8, 1, 1): 1}


def all_stack_inputs():
    """(B, F, H, L, T, P) of every stack-shaped input above, each once."""
    out = [(B, F, H, 1, T, P_SMALL) for (B, F, H, T) in LAYER_CASES]
    out += [(B, F, H, L, T, P_SMALL) for (B, F, H, L, T) in STACK_CASES]
    out += sorted({(B, 40, 768, 3, T, P_768) for (B, T, _) in H768_CASES})
    return out


@functools.lru_cache(maxsize=None)
def inputs(B, F, H, L, T, P):
    """(state dict of fp32 master weights, frames x [B,T,F], demb [B,P]) of a case."""
    shift = SEED_SHIFT.get((B, F, H, L, T), 0)
    sd = recipe.make_weights(1000 + B + 3 * F + 5 * H + 7 * L + 11 * T + shift, F, H, L, P, scale=3.0)
    x = recipe.make_frames(2000 + B * T + F + H + shift, B, T, F)
    demb = np.random.default_rng(3000 + B + T + P).standard_normal((B, P)).astype(np.float32)
    return sd, x, demb


def layer_weights(sd, L):
    """[(w_ih, w_hh, b_ih, b_hh)] * L (numpy fp32), w_p, b_p."""
    ws = [tuple(sd[f"LSTM_stack.{n}_l{l}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
          for l in range(L)]
    return ws, sd["projection.weight"], sd["projection.bias"]
