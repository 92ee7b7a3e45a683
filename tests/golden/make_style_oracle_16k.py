"""Record oracle/effects.py's 16 kHz outputs of styles 2, 3 and 4 (the chorus boards) as they were before the
chorus history was padded by the delay line's real maximum: tests/test_style_envelope_cpu.py asserts that the
edited oracle reproduces them bit for bit.  Ran once, on the oracle of the parent commit; running it again on
a later oracle records that oracle's outputs and proves nothing.

    python tests/golden/make_style_oracle_16k.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import effects as oe  # noqa: E402


def clips(n, L, seed):
    r = np.random.default_rng(seed)
    t = np.arange(L) / 16000
    x = 0.3 * np.sin(2 * np.pi * r.uniform(100, 3000, (n, 1)) * t) + r.normal(0, 0.05, (n, L))
    x[1] *= 4.0
    return np.clip(x, -1, 1).astype(np.float32)


if __name__ == "__main__":
    x = clips(2, 2500, 20)
    np.savez_compressed(os.path.join(HERE, "style_oracle_16k.npz"), x=x, style2=oe.style2(x), style3=oe.style3(x),
                        style4=oe.style4(x))
