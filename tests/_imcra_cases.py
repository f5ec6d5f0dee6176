"""The kernel-against-restatement inputs of tests/test_gpu_imcra.py, shared with
tools/imcra_tolerance.py, which walks exactly these on the CPU."""

import numpy as np

# (T, B, S).  T: 1, 2 and 4; both sides of the first sub-window switch (V = 15:
# frame 14 rolls, frame 15 is the first to read the result) and of the kernel's
# 8-frame prefetch blocks (frames [1, 1 + 8 ((T - 2) // 8)) run in whole blocks:
# none below T = 10, one at 10 and 17, two at 18); both sides of the whole
# window (U V = 120) and the first overwritten slot (136); one long case.
# B: the ends 33 and 2049, the grid's 257, 129 (no multiple of the wave), and
# the kernel's 62-bin blocks: 63 and 125 leave one bin to the last block, 124
# fills two blocks exactly.  S: 1 and 3.
KERNEL_CASES = [(1, 33, 1), (2, 33, 1), (4, 129, 1), (10, 33, 1), (14, 257, 1), (15, 257, 3),
                (16, 257, 1), (17, 129, 1), (18, 63, 1), (18, 124, 1), (18, 125, 3), (30, 257, 1),
                (31, 33, 3), (120, 257, 1), (121, 129, 1), (136, 257, 1), (253, 2049, 1)]
SHORT_CASES = [c for c in KERNEL_CASES if c[0] <= 31]
# the short cases run a second time with a window of U V = 8 frames and lower
# thresholds, so that the roll-over of the window, I = 0 and a fractional qh all
# occur within 18 frames
SMALL = dict(sub_windows=2, sub_frames=4, gamma0=2.0, zeta0=1.3)
# every field changed
OTHER = dict(alpha=0.85, alpha_s=0.8, alpha_d=0.9, beta=1.2, b_min=1.4, gamma0=3.5, gamma1=2.5,
             zeta0=1.5, xi_min_db=-12.0, sub_windows=5, sub_frames=6)


def step_power(T, B, S):
    """Exponential power, multiplied by 100 from frame T // 2 on."""
    t = np.arange(T)[None, :, None]
    return np.random.default_rng(T).exponential(size=(S, T, B)) * np.where(t < T // 2, 1, 100)


def other_power():
    power = np.random.default_rng(5).exponential(size=(2, 70, 129))
    power[:, 30:50] *= 40.0
    return power


def all_inputs():
    """(name, power, eps, params) of every kernel-against-restatement comparison."""
    for T, B, S in KERNEL_CASES:
        yield f"T={T} B={B} S={S}", step_power(T, B, S), 1e-10, {}
    for T, B, S in SHORT_CASES:
        yield f"T={T} B={B} S={S} SMALL", step_power(T, B, S), 1e-12, SMALL
    yield "non-default", other_power(), 1e-12, OTHER
