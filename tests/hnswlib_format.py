"""A pure-Python reader of hnswlib's saveIndex container (0.7.x / 0.8.x
layout, restated in DESIGN.md §HNSW), independent of dg_hnsw_core.h: the
tests parse the library's bytes with it and build malformed variants from
the offsets it reports.  Little-endian; size_t and labels 8 bytes; tableint
and list headers uint32."""
import struct

import numpy as np

HEADER = struct.Struct("<6QiI3QdQ")  # 96 bytes


def parse(buf):
    """-> dict of the header fields, per-node arrays and the byte offsets of
    the level-0 records (rec_off) and of each node's linkListSize (ll_off)."""
    (off_l0, max_elements, n, per_elem, label_off, off_data, maxlevel, enter,
     max_m, max_m0, m, mult, efc) = HEADER.unpack_from(buf, 0)
    assert off_l0 == 0
    assert off_data == 4 + 4 * max_m0
    assert per_elem == label_off + 8
    d = (label_off - off_data) // 4
    assert label_off == off_data + 4 * d
    pos = HEADER.size
    cnt0 = np.zeros(n, np.int32)
    deleted = np.zeros(n, np.uint8)
    links0 = np.zeros((n, max_m0), np.uint32)
    rows = np.zeros((n, d), np.float32)
    labels = np.zeros(n, np.int64)
    rec_off = []
    for i in range(n):
        rec_off.append(pos)
        (h,) = struct.unpack_from("<I", buf, pos)
        cnt0[i] = h & 0xffff
        deleted[i] = (h >> 16) & 1
        links0[i] = np.frombuffer(buf, "<u4", max_m0, pos + 4)
        rows[i] = np.frombuffer(buf, "<f4", d, pos + off_data)
        (labels[i],) = struct.unpack_from("<q", buf, pos + label_off)
        pos += per_elem
    levels = np.zeros(n, np.int32)
    upper = []  # per node: list over levels 1.. of (count, links[max_m])
    ll_off = []
    per_list = 4 + 4 * max_m
    for i in range(n):
        ll_off.append(pos)
        (sz,) = struct.unpack_from("<I", buf, pos)
        pos += 4
        assert sz % per_list == 0
        levels[i] = sz // per_list
        lists = []
        for _ in range(levels[i]):
            (h,) = struct.unpack_from("<I", buf, pos)
            lists.append((h & 0xffff,
                          np.frombuffer(buf, "<u4", max_m, pos + 4).copy()))
            pos += per_list
        upper.append(lists)
    assert pos == len(buf), (pos, len(buf))
    return dict(max_elements=max_elements, n=n, d=d, maxlevel=maxlevel,
                enterpoint=enter, maxM=max_m, maxM0=max_m0, M=m, mult=mult,
                ef_construction=efc, cnt0=cnt0, deleted=deleted,
                links0=links0, rows=rows, labels=labels, levels=levels,
                upper=upper, rec_off=rec_off, ll_off=ll_off,
                per_elem=per_elem, label_off=label_off, off_data=off_data)


def patch(buf, offset, fmt, value):
    """A copy of buf with struct-format fmt written at offset."""
    b = bytearray(buf)
    struct.pack_into(fmt, b, offset, value)
    return bytes(b)


# byte offsets of the header fields
H_MAX_ELEMENTS, H_COUNT, H_PER_ELEM, H_LABEL_OFF, H_OFF_DATA = 8, 16, 24, 32, 40
H_MAXLEVEL, H_ENTER, H_MAXM, H_MAXM0, H_M = 48, 52, 56, 64, 72
