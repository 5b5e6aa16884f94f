"""numpy restatement of dspn_jpeg_scan_index (include/dspn_jpeg.h) for tests/test_jpeg_restart_host.py: where the restart
intervals of a scan start, found from the 0xFF bytes alone, and the Huffman tables as the DHT segments carry them."""
import numpy as np

import ref_jpeg


def raw_tables(data):
    """{(class, id): (16 counts, values)} of every DHT segment in front of SOS"""
    out, p = {}, 2
    while True:
        assert data[p] == 0xFF
        while data[p] == 0xFF:
            p += 1
        m = data[p]
        L = (data[p + 1] << 8) | data[p + 2]
        seg = data[p + 3:p + 1 + L]
        p += 1 + L
        if m == 0xC4:
            q = 0
            while q < len(seg):
                counts = np.frombuffer(seg[q + 1:q + 17], np.uint8)
                n = int(counts.sum())
                out[(seg[q] >> 4, seg[q] & 15)] = (counts, np.frombuffer(seg[q + 17:q + 17 + n], np.uint8))
                q += 17 + n
        elif m == 0xDA:
            return out


def index(data):
    """-> dict: scan_pos, offsets (uint32, relative to scan_pos: the start of every interval's data and the closing
    offset), interval, mcus_w, mcus_h, td, ta, tables"""
    P = ref_jpeg.parse(data)
    a = np.frombuffer(data, np.uint8)
    s = P["scan_pos"]
    ff = np.flatnonzero(a[s:-1] == 0xFF) + s
    nxt = a[ff + 1]
    markers = ff[(nxt != 0x00) & (nxt != 0xFF)]                # the last 0xFF in front of a marker code
    offsets = [0]
    for q in markers:
        code = int(a[q + 1])
        if 0xD0 <= code <= 0xD7:
            offsets.append(int(q) + 2 - s)
            continue
        start = int(q)
        while start - 1 >= s and a[start - 1] == 0xFF:         # fill bytes belong to the marker
            start -= 1
        offsets.append(start - s)
        break
    return {"scan_pos": s, "offsets": np.array(offsets, np.uint32), "interval": P["restart_interval"], "mcus_w": P["mcux"],
            "mcus_h": P["mcuy"], "td": P["td"], "ta": P["ta"], "tables": raw_tables(data)}
