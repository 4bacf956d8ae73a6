"""Wide items (an item spread over several plaintexts, pirgpu_params.plaintexts_per_item) -- the host-side contract:
parameter arithmetic, struct layout, exported symbols.  No GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

from pir_amd import capi
from pir_amd import parameters as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def enc24():
    return P.generate_encryption_params(4096, 24)


def test_opt_in_gives_planes():
    pp = P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=4)
    assert pp.plaintexts_per_item == pp.planes == 3          # ceil(30000 / 11776)
    assert pp.max_bytes_per_plaintext == 11776               # N * 23 / 8
    assert pp.items_per_plaintext == 1
    assert pp.num_pt == 20
    assert pp.dimensions == [5, 4]
    assert pp.bytes_per_item == 30000
    assert [(r.start, r.stop) for r in map(pp.plane_bytes, range(3))] == [(0, 11776), (11776, 23552), (23552, 30000)]
    # the index arithmetic of a request sees one item per plaintext
    assert pp.calculate_indices(13) == [3, 1] and pp.calculate_item_offset(13) == 0


def test_default_still_refuses_an_oversized_item():
    with pytest.raises(ValueError, match="^Cannot fit an item within one plaintext$"):
        P.create_pir_parameters(20, 30000, 2, enc24())
    with pytest.raises(ValueError, match="^Cannot fit an item within one plaintext$"):
        P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=1)


def test_too_few_planes_allowed_raises():
    with pytest.raises(ValueError, match="Cannot fit an item within 2 plaintexts"):
        P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=2)
    assert P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=3).planes == 3


def test_item_that_fits_one_plaintext_is_unchanged_by_the_argument():
    a = P.create_pir_parameters(3000, 288, 2, enc24())
    b = P.create_pir_parameters(3000, 288, 2, enc24(), max_plaintexts_per_item=4)
    assert a == b and b.planes == 1 and b.items_per_plaintext == 40
    # exactly one plaintext's worth is still one plane; one byte more is two
    assert P.create_pir_parameters(5, 11776, 1, enc24(), max_plaintexts_per_item=4).planes == 1
    assert P.create_pir_parameters(5, 11777, 1, enc24(), max_plaintexts_per_item=4).planes == 2


def test_explicit_bits_per_coeff_sets_the_plane_size():
    pp = P.create_pir_parameters(10, 12000, 1, enc24(), bits_per_coeff_=16, max_plaintexts_per_item=2)
    assert pp.max_bytes_per_plaintext == 8192 and pp.planes == 2


def test_struct_layout_and_new_field_offset_match_the_header():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include "pirgpu.h"\nint main(){printf("%zu %zu %zu", '
                             'sizeof(pirgpu_params), __builtin_offsetof(pirgpu_params, plaintexts_per_item), '
                             '__builtin_offsetof(pirgpu_params, slot_end));return 0;}')
        exe = os.path.join(d, "s")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        size, off_planes, off_slot_end = map(int, subprocess.run([exe], capture_output=True, text=True).stdout.split())
    assert C.sizeof(capi.Params) == size
    assert capi.Params.plaintexts_per_item.offset == off_planes
    assert capi.Params.slot_end.offset == off_slot_end
    assert off_planes == off_slot_end + 4                     # the trailing field


def test_make_params_carries_the_field():
    wide = P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=4)
    assert capi.make_params(wide).plaintexts_per_item == 3
    assert capi.make_params(P.create_pir_parameters(3000, 288, 2, enc24())).plaintexts_per_item == 1


def test_pirgpu_planes_is_exported_and_bound():
    lib = capi.load()
    assert hasattr(lib, "pirgpu_planes")
    assert "pirgpu_planes" in capi.SIGNATURES
    assert "pirgpu_planes" in open(os.path.join(ROOT, "include", "pirgpu.h")).read()
    assert lib.pirgpu_planes(None) == 0                       # null context, like the other accessors


def test_client_reply_count_follows_planes():
    import pir_amd
    wide = P.create_pir_parameters(20, 30000, 2, enc24(), max_plaintexts_per_item=4)
    one = P.create_pir_parameters(20, 0, 2, enc24())
    cw = pir_amd.PIRClient.Create(wide, seed=b"w")
    c1 = pir_amd.PIRClient.Create(one, seed=b"w")
    assert cw.reply_ct_count == 3 * c1.reply_ct_count == 24
    assert cw.query_ct_count == c1.query_ct_count
