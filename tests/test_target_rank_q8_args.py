"""functional.target_ranks_q8: every argument check comes before the device is looked at (CPU tensors), under its own name."""
import pytest
import torch

import q8_ref


@pytest.mark.parametrize("case,exc", [("dtype", TypeError), ("stride", ValueError), ("width", NotImplementedError),
                                      ("P17", ValueError), ("range", ValueError), ("exclude", ValueError),
                                      ("X", NotImplementedError)])
def test_argument_errors_before_any_launch(case, exc):
    from torecsys_amd import functional as F_
    E = 6 if case == "width" else 32
    a, q = torch.zeros(4, E), torch.zeros(200, q8_ref.stride(E), dtype=torch.uint8)
    if case == "dtype":
        q = q.to(torch.int8)
    if case == "stride":
        q = torch.zeros(200, 64, dtype=torch.uint8)
    y = torch.zeros(4, 17 if case == "P17" else 2, dtype=torch.int64)
    ex = {"exclude": torch.zeros(3, 2, dtype=torch.int64), "X": torch.zeros(4, 1025, dtype=torch.int64)}.get(case)
    with pytest.raises(exc, match="target_ranks_q8"):
        F_.target_ranks_q8(a, None, q, E, y, target_hi=201 if case == "range" else None, exclude=ex)
