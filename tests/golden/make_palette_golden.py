"""Writes cityscapes_palette.json: trainId, name and colour of every label of the reference's dataset/cs_labels.py with
0 <= trainId < 255 -- the rows its display code puts into the 256-entry colour table (multi_eval.py:39-44,
detect/multitask_detector.py:352-357).

    python tests/golden/make_palette_golden.py <root of a liangfu/dspnet checkout>

The label table is loaded from that checkout when the fixture is generated (the module imports under Python 3 and
needs nothing else); nothing of it is kept here but the three fields of those rows.  A later label with the same trainId
replaces an earlier one, as the assignments of the display code do."""
import importlib.util
import json
import os
import sys


def rows(reference_root):
    path = os.path.join(reference_root, "dataset", "cs_labels.py")
    spec = importlib.util.spec_from_file_location("cs_labels", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    table = {}
    for label in mod.labels:
        if 0 <= label.trainId < 255:
            table[int(label.trainId)] = {"trainId": int(label.trainId), "name": str(label.name),
                                         "color": [int(v) for v in label.color]}
    return [table[k] for k in sorted(table)]


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cityscapes_palette.json")
    with open(out, "w") as f:
        json.dump({"source": "dataset/cs_labels.py, labels with 0 <= trainId < 255", "labels": rows(sys.argv[1])}, f, indent=1)
        f.write("\n")
