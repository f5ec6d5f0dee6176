"""The shapes, signals and error bound of the STFT front-end tests, shared by
tests/test_stft_host.py (the fp64 oracle against a long-double direct DFT) and
tests/test_gpu_stft.py (cse_stft against the oracle), so both walk the same
cases.  Host-only: numpy, no device, no torch.

A case is (n_fft, hop, length, n_sig, note).  cse_stft (csrc/cse_stft.hip) holds
three transforms behind one switch; form(n_fft) names the one a case runs:
  radix2  stft_kernel<N>, N in 64 .. 4096 without 512: radix 2 in LDS, 4 frames
          per workgroup up to 1024 (a partial last block where T % 4 != 0), one
          above;
  r512    stft512_kernel: the register DFT16 x 16, 16 frames per workgroup, 16
          lanes per frame (whole 16-lane groups leave early where T % 16 != 0);
  dft     stft_dft_kernel: the direct DFT of every other even size, one frame
          per workgroup, B = n_fft/2 + 1 bins strided over 256 threads.
T = 1 + length // hop frames.
"""

import numpy as np

SEED = 20260


def form(n_fft):
    if n_fft & (n_fft - 1):
        return "dft"
    return "r512" if n_fft == 512 else "radix2"


def _length_edges(n_fft, hop, t, k):
    """Lengths at which the reflect padding or the frame count changes: 1 and 2
    (every sample is the padding of every other), around n_fft/2 (below it the
    padding reflects more than once), a frame that ends exactly at the last
    sample (length == t hop + n_fft/2: the last frame of the `inside` path), a
    whole number of hops (the frame count steps there) and one less."""
    h = n_fft // 2
    out = [(1, "len 1"), (2, "len 2"), (h - 1, "len n_fft/2 - 1: reflects twice"),
           (h, "len n_fft/2"), (h + 1, "len n_fft/2 + 1"),
           (t * hop + h, f"frame {t} ends at the last sample"),
           (k * hop, f"len = {k} hops"), (k * hop - 1, f"len = {k} hops - 1")]
    return [(n_fft, hop, length, 1, note) for length, note in out]


CASES = [
    # radix 2, every instantiation; T % 4 != 0 up to 1024 (a partial last block)
    (64, 16, 1000, 1, "radix 2, T = 63"),
    (128, 32, 1100, 1, "radix 2, T = 35"),
    (128, 32, 1000, 1, "radix 2, T = 32: whole blocks only"),
    (256, 64, 1400, 1, "radix 2, T = 22"),
    (1024, 256, 3400, 1, "radix 2, T = 14"),
    (2048, 512, 5000, 1, "radix 2, one frame per workgroup, T = 10"),
    (4096, 1024, 9000, 1, "radix 2, one frame per workgroup, T = 9"),
    # 512: T % 16 in {0, 1, 15}
    (512, 128, 2000, 1, "512, T = 16"),
    (512, 128, 2100, 1, "512, T = 17: one frame in the last block"),
    (512, 128, 1800, 1, "512, T = 15: one 16-lane group returns early"),
    # the direct DFT; 4094 is the largest size it takes (B = 2048)
    (66, 22, 500, 1, "direct DFT, B = 34"),
    (400, 160, 2000, 1, "direct DFT, B = 201"),
    (4000, 1000, 9000, 1, "direct DFT above 2048, B = 2001"),
    (4094, 2047, 9000, 1, "direct DFT, the largest size, B = 2048"),
    # hop edges
    (64, 1, 200, 1, "hop 1"),
    (130, 1, 200, 1, "hop 1, direct DFT"),
    (64, 64, 500, 1, "hop = n_fft"),
    (512, 512, 3000, 1, "hop = n_fft"),
    (400, 400, 2000, 1, "hop = n_fft"),
    (4096, 4096, 13000, 1, "hop = n_fft"),
    # a frame that ends exactly at the last sample, away from the three below
    (256, 64, 768, 1, "frame 10 ends at the last sample"),
    (64, 16, 5, 1, "len 5"),
]
CASES += _length_edges(64, 16, 5, 10)
CASES += _length_edges(512, 128, 6, 10)
CASES += _length_edges(400, 160, 4, 10)
CASES += [
    # three different signals of an odd length: rows 1 and 2 start off 16 bytes
    (64, 16, 333, 3, "3 signals"),
    (512, 128, 1001, 3, "3 signals"),
    (400, 160, 777, 3, "3 signals"),
    (2048, 512, 4501, 3, "3 signals, one frame per workgroup"),
]


def case_id(case):
    n_fft, hop, length, n_sig, _ = case
    return f"{n_fft}/{hop} len {length}" + (f" x{n_sig}" if n_sig > 1 else "")


def signals(case):
    """[n_sig, length] fp64: white noise plus a linear ramp of another slope per
    signal.  The ramp breaks every symmetry: a frame mirrored, or loaded one
    sample off, changes by far more than the bound."""
    n_fft, hop, length, n_sig, _ = case
    rng = np.random.default_rng([SEED, n_fft, hop, length, n_sig])
    x = 0.25 * rng.standard_normal((n_sig, length))
    ramp = (np.arange(length, dtype=np.float64) + 1.0) / length
    return x + (0.5 + 0.25 * np.arange(n_sig))[:, None] * ramp[None, :]


def hann(n_fft):
    """The periodic Hann window, 0.5 - 0.5 cos(2 pi n / N)."""
    n = np.arange(n_fft, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * n / n_fft)


def padded(x, n_fft):
    """x with n_fft/2 reflected samples at either end, by numpy's own np.pad
    (which reflects again where the signal is shorter than the padding), not by
    the oracle's index map: the two are compared in the host test."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] == 1:  # one sample reflects onto itself
        return np.repeat(x, n_fft + 1, axis=-1)
    pad = [(0, 0)] * (x.ndim - 1) + [(n_fft // 2, n_fft // 2)]
    return np.pad(x, pad, mode="reflect")


def frames_windowed(x, n_fft, hop):
    """[T, n_fft]: the windowed frames xw of the centred, reflect-padded STFT of
    one signal x [length], T = 1 + length // hop."""
    p = padded(x, n_fft)
    T = 1 + x.shape[-1] // hop
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    return p[idx] * hann(n_fft)[None, :]


def stft_bound(frames_windowed, n_fft):
    """The absolute tolerance of a frame's spectrum, per frame:

        2 n_fft 2**-53 sum_n |xw_n|

    X_k = sum_n xw_n w^{kn} summed in fp64 in any order has a forward error of
    at most (n_fft - 1) u sum_n |xw_n w^{kn}| (1 + O(u)) in each component,
    u = 2**-53, and twiddles good to an ulp add u sum_n |xw_n|; |w| = 1, so
    n_fft u sum |xw_n| covers the direct DFT, and the FFT forms (log2 n_fft
    levels instead of n_fft terms) a fortiori.  The factor 2 leaves the same
    again for the reference's own error and for the window's rounding.
    Derived, not measured; no figure from the device enters it."""
    fw = np.asarray(frames_windowed)
    return 2.0 * n_fft * 2.0 ** -53 * np.sum(np.abs(fw), axis=-1, dtype=np.float64)


def direct_dft_longdouble(xw):
    """The direct DFT of one windowed frame xw [N] summed in np.longdouble,
    bins 0 .. N/2: (re, im) as longdouble.  The twiddles come from the
    long-double cos / sin of 2 pi (kn mod N) / N."""
    xw = np.asarray(xw, dtype=np.longdouble)
    N = xw.shape[0]
    ang = 2 * np.pi * np.arange(N, dtype=np.longdouble) / np.longdouble(N)
    c, s = np.cos(ang), np.sin(ang)
    k = np.arange(N // 2 + 1)[:, None]
    m = (k * np.arange(N)[None, :]) % N
    return (c[m] * xw[None, :]).sum(axis=1), -(s[m] * xw[None, :]).sum(axis=1)


# The analytic pin: x = A cos(2 pi k0 n / N) under the periodic Hann window is
# three lines whatever the frame's position: |X[k0]| = A N / 4 and
# |X[k0 +- 1]| = A N / 8 (the window's three coefficients 1/2, -1/4, -1/4 on
# the line of weight A N / 2); with 2 <= k0 <= N/2 - 2 the image at -k0 reaches
# none of them, and every other bin is zero.  (N, hop, k0).
PIN_A = 0.7
PIN_CASES = [(64, 16, 5), (512, 128, 37), (400, 160, 29), (4096, 1024, 301)]


def pin_signal(N, k0, length):
    """A cos(2 pi k0 n / N), the phase reduced mod N in integers before the
    cosine, so that sample 40000 is as good as sample 3."""
    n = np.arange(length)
    return PIN_A * np.cos(2.0 * np.pi * ((k0 * n) % N).astype(np.float64) / N)


def pin_length(N, hop):
    return 5 * N + hop // 2 + 3


def pin_interior(N, hop, length):
    """The frames that touch no padding: 0 <= t hop - N/2 and t hop + N/2 <= length."""
    t = np.arange(1 + length // hop)
    return t[(t * hop - N // 2 >= 0) & (t * hop + N // 2 <= length)]


def pin_expected(N, k0):
    """|X| per bin, [N/2 + 1]."""
    e = np.zeros(N // 2 + 1)
    e[k0] = PIN_A * N / 4.0
    e[k0 - 1] = e[k0 + 1] = PIN_A * N / 8.0
    return e


# cse_istft_norm shapes: (n_fft, hop, length)
NORM_CASES = [(512, 128, 2100), (1024, 256, 3400), (64, 1, 200), (400, 160, 2000),
              (4096, 4096, 13000), (64, 16, 1), (64, 16, 31)]


def istft_norm_ref(n_fft, hop, length):
    """(1 / wss [length] fp64 with 1 where wss <= tiny, the mask of those
    samples): the window-sum-square normalisation of librosa's istft over
    nf = min(T, ceil((length + n_fft) / hop)) frames."""
    import oracle
    T = 1 + length // hop
    nf = min(T, -(-(length + n_fft) // hop))
    wss = oracle.window_sumsquare(nf, hop, n_fft)[n_fft // 2:n_fft // 2 + length]
    # past the last frame's end nothing is summed (fix_length pads with zeros)
    wss = np.concatenate([wss, np.zeros(length - len(wss))])
    dead = wss <= np.finfo(float).tiny
    return np.where(dead, 1.0, 1.0 / np.where(dead, 1.0, wss)), dead
