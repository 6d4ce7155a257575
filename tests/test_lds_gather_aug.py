"""LDS bank-conflict model (tools/lds_bank_model.py) of the augmenting batch gather's tile
transpose (csrc/kernels/gather.h): the padded row pitches make the row writes and the
transposed reads conflict-free where the unpadded tile is a 32- / 16-way conflict."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import lds_bank_model as m  # noqa: E402


def test_image_tile_pitches_are_conflict_free():
    # nw = dwords per pixel: 2 (Cpad 4, 16 bit), 4 (Cpad 8 in 16 bit, Cpad 4 in fp32)
    assert m.check_gather_aug(2) == (1, 1)
    assert m.check_gather_aug(4) == (1, 1)
    # fp32 with 8 channels (32-byte pixels): conflict-free reads; 8 lanes of a 16-byte store
    # group are 32 bytes apart and wrap the 32 store banks twice
    assert m.check_gather_aug(8) == (2, 1)


def test_unpadded_tile_would_serialise_the_transposed_reads():
    assert m.check_gather_aug(2, pad=0) == (1, 32)
    assert m.check_gather_aug(4, pad=0) == (1, 16)


def test_target_plane_pitch():
    assert m.check_gather_aug_target() == (1, 1)
    assert m.check_gather_aug_target(pitch=32) == (1, 32)
