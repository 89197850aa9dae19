"""CPU: the numpy restatement of the device sums' one shape (tests/sums_common.py) against the same shape written out in plain Python
floats (ndt_common.shape_sums_plain) -- at one slot, one slot past a workgroup's threads and one slot past a segment."""
import numpy as np
import pytest

import ndt_common as nd
import sums_common as sc


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_the_shape_in_numpy_is_the_shape_in_plain_floats(n):
    """Terms of mixed sign over twelve binades, a fifth of them +0.0 as a dead term's: any other order of adding rounds differently."""
    rs = np.random.RandomState(n)
    C = rs.standard_normal((n, 7, 3, 28)) * 2.0 ** rs.randint(-6, 6, (n, 7, 3, 28))
    C[rs.uniform(size=(n, 7, 3)) < 0.2] = 0.0
    a = sc.shape_sums(C.reshape(n, 21, 28))
    assert a.shape == (28,) and a.tobytes() == nd.shape_sums_plain(C).tobytes()
    assert nd.shape_sums(C).tobytes() == a.tobytes()
    if n > 1:      # (the order matters at these sizes: the pin can tell the shape from a plain ascending sum)
        assert np.any(a != C.reshape(-1, 28).cumsum(0)[-1])
