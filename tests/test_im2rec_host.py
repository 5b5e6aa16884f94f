"""dataset/im2rec.py without a GPU: the .lst reader and the pass-through writer (file bytes packed as they are)."""
import os

import numpy as np
import pytest

import jpeg_cases as jc
from dspnet_amd.dataset import im2rec, recordio


def test_read_list_takes_the_references_format(tmp_path):
    p = tmp_path / "a.lst"
    p.write_text("7\t1.000000\tx/a.jpg\n\n3\t2.000000\t6.000000\t-1.000000\tdir with space/b.jpg\n")
    assert im2rec.read_list(str(p)) == [(7, [1.0], "x/a.jpg"), (3, [2.0, 6.0, -1.0], "dir with space/b.jpg")]
    p.write_text("7\tx/a.jpg\n")
    with pytest.raises(ValueError, match="2 columns"):
        im2rec.read_list(str(p))
    p.write_text("7\tcar\tx/a.jpg\n")
    with pytest.raises(ValueError, match="a.lst:1"):
        im2rec.read_list(str(p))


def test_pass_through_packs_the_file_bytes_in_list_order(tmp_path):
    root = tmp_path / "images"
    root.mkdir()
    files = {"a.jpg": jc.stream("17x33-ss2-q90-std-noise"), "b.jpg": jc.stream("8x8-grey-q90-noise"), "c.bin": b"\x00\x01not an image"}
    for name, data in files.items():
        (root / name).write_bytes(data)
    prefix = str(tmp_path / "set")
    with open(prefix + ".lst", "w") as f:
        f.write("5\t1.000000\t2.000000\tb.jpg\n2\t4.000000\ta.jpg\n9\t0.500000\t0.250000\tc.bin\n")
    assert im2rec.write_records(prefix, str(root), pass_through=True, batch=2) == 3
    rec = recordio.MXIndexedRecordIO(prefix + ".idx", prefix + ".rec", "r")
    assert rec.keys == [5, 2, 9]
    for key, name, label in ((5, "b.jpg", [1.0, 2.0]), (2, "a.jpg", 4.0), (9, "c.bin", [0.5, 0.25])):
        header, payload = recordio.unpack(rec.read_idx(key))
        assert payload == files[name] and header.id == key
        np.testing.assert_array_equal(header.label, np.float32(label))
    rec.close()
    assert im2rec.write_records(prefix, str(root), pack_label=False, pass_through=True) == 3
    rec = recordio.MXIndexedRecordIO(prefix + ".idx", prefix + ".rec", "r")
    assert [recordio.unpack(rec.read_idx(k))[0].label for k in (5, 2, 9)] == [1.0, 4.0, 0.5]
    rec.close()
    os.remove(str(root / "a.jpg"))
    with pytest.raises(OSError):
        im2rec.write_records(prefix, str(root), pass_through=True)
