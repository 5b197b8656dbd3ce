"""Bit-for-bit comparison of float arrays, shared by the per-call device tests."""
import numpy as np

F = np.float32


def assert_same_bits(name, got, want, *inputs):
    """got, want: equal-shaped float32 or float64 arrays, one row per case.  Equal bit for bit; two NaNs count as equal (their sign
    and payload are the hardware's).  On failure: the first five cases, inputs and both results in hex."""
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    got = np.ascontiguousarray(got).reshape(len(got), -1); want = np.ascontiguousarray(want, got.dtype).reshape(got.shape)
    bad = np.flatnonzero(((got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want))).any(axis=1))
    hx = lambda v: " ".join(f"{int(w):x}" for w in np.atleast_1d(v))
    lines = [f"in {' '.join(hx(np.asarray(a, F)[k].view(np.uint32)) for a in inputs)}: device {hx(got[k].view(u))} host {hx(want[k].view(u))}"
             for k in bad[:5]]
    assert len(bad) == 0, f"{name}: {len(bad)} of {len(got)} cases differ\n" + "\n".join(lines)
    return len(got)
