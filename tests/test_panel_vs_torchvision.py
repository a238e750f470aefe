"""Pin-on-arrival of the panel's grid geometry: torchvision is not installed where this project is built, so
tests/panel_ref.py restates ``torchvision.utils.make_grid`` from its published source.  This file skips without
``torchvision``; with it, it compares the restatement's placement with the real function."""
import numpy as np
import pytest
import torch

import panel_ref as R

vutils = pytest.importorskip("torchvision.utils", reason="torchvision is not installed: make_grid stays pinned to its published source only")


@pytest.mark.parametrize("K,nrow,padding,pad_value", [(1, 8, 2, 0), (4, 4, 2, 0), (16, 4, 2, 0), (20, 4, 2, 0), (5, 8, 2, 255),
                                                      (9, 8, 2, 0), (7, 3, 0, 0), (7, 3, 1, 255), (6, 1, 3, 0), (3, 2, 2, 7)])
def test_place_is_make_grid(K, nrow, padding, pad_value):
    cells = np.random.default_rng(K * 10 + nrow).integers(0, 256, (K, 3, 5, 7), dtype=np.uint8)
    want = vutils.make_grid(torch.from_numpy(cells), nrow=nrow, padding=padding, pad_value=pad_value).numpy()
    assert np.array_equal(R.place(cells, nrow, padding, pad_value), want)


def test_one_channel_cells_fill_three():
    cells = np.random.default_rng(3).integers(0, 256, (4, 1, 5, 7), dtype=np.uint8)
    want = vutils.make_grid(torch.from_numpy(cells), nrow=4).numpy()
    assert np.array_equal(R.place(np.broadcast_to(cells, (4, 3, 5, 7)), 4), want)
