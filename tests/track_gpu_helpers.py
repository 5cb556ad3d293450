"""What the GPU tests of the tracking layer share (tests/test_gpu_track*.py): host arrays onto the device, and the
uneven pieces a stream is pushed in."""
import numpy as np
import torch


def dev(cuda, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)


def pieces_of(T):
    """Uneven pieces 1, 2, 0, 3, ... that add up to T: the first is shorter than max_gap + 1 for max_gap >= 1."""
    out, want = [], [1, 2, 0, 3, 1, 2]
    while sum(out) < T:
        out.append(min(want[len(out) % len(want)], T - sum(out)))
    return out
