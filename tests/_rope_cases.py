"""The RoPE parameter rows shared by tests/test_gpu_rope.py (every fused RoPE site against the oracle) and
tests/test_oracle_vs_ref.py (the oracle against the reference on the same rows), with the YaRN helpers both need."""
import collections
import math

import numpy as np

Row = collections.namedtuple("Row", "id dh n_dims mode freq_base freq_scale ext_factor attn_factor n_ctx_orig with_ff")

ROWS = [
    Row("default",           128, 128, 0, 5e5, 1.0,  0.0, 1.0, 8192, True),
    Row("linear",            128, 128, 0, 1e4, 0.25, 0.0, 1.0, 4096, False),
    Row("yarn-neox",         128, 128, 2, 1e6, 0.25, 1.0, 1.1, 4096, False),
    Row("yarn-ff-partial",   128, 64,  0, 1e4, 0.5,  1.0, 1.0, 4096, True),
    Row("yarn-neox-64",      64,  64,  2, 1e6, 0.25, 1.0, 1.1, 4096, False),
    Row("partial-64",        64,  32,  0, 1e4, 1.0,  0.0, 1.0, 8192, False),
    Row("yarn-neox-partial", 128, 96,  2, 1e4, 0.25, 1.0, 1.0, 4096, True),
]
ROW_IDS = [r.id for r in ROWS]
BETA_FAST, BETA_SLOW = 32.0, 1.0
POSITIONS = [0, 37, 32765, 131068]          # T = 4 tokens from each: the far ones cross 32768 and end at 131071


def yarn_corr(n_dims, freq_base, n_ctx_orig, beta_fast=BETA_FAST, beta_slow=BETA_SLOW):
    """corr0 / corr1 of pm_rope_params (ggml_rope_yarn_corr_dims): pairs below corr0 keep the unscaled angle (mix = ext_factor), pairs above
    corr1 the scaled one (mix = 0), the ramp lies between."""
    def corr_dim(n_rot):
        return n_dims * math.log(n_ctx_orig / (n_rot * 2 * math.pi)) / (2 * math.log(freq_base))
    return max(0.0, math.floor(corr_dim(beta_fast))), min(float(n_dims - 1), math.ceil(corr_dim(beta_slow)))


def assert_three_yarn_regimes(n_dims, freq_base, n_ctx_orig):
    """A YaRN case is worth its name only if its pairs fall into all three regimes: some before the ramp, some on it, some after it."""
    c0, c1 = yarn_corr(n_dims, freq_base, n_ctx_orig)
    assert 0 < c0 < c1 < n_dims / 2 - 1, (n_dims, freq_base, n_ctx_orig, c0, c1)
    return c0, c1


for _r in ROWS:
    if _r.ext_factor:
        assert_three_yarn_regimes(_r.n_dims, _r.freq_base, _r.n_ctx_orig)


def rope_kw(row):
    """The row as the keywords that oracle.rope and the prima_cpp_amd.ops wrappers share (freq_factors apart)."""
    return dict(n_dims=row.n_dims, mode=row.mode, n_ctx_orig=row.n_ctx_orig, freq_base=row.freq_base, freq_scale=row.freq_scale,
                ext_factor=row.ext_factor, attn_factor=row.attn_factor, beta_fast=BETA_FAST, beta_slow=BETA_SLOW)


def magnitude(row):
    """ms: what the rotation multiplies every rotated pair with (1 without YaRN and attn_factor)."""
    return row.attn_factor * (1.0 + 0.1 * math.log(1.0 / row.freq_scale) if row.ext_factor else 1.0)


def freq_factors(row):
    return (1 + np.random.default_rng(7).uniform(0, 7, row.dh // 2)).astype(np.float32) if row.with_ff else None
