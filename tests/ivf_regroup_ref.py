"""The regroup of IVF storage restated in numpy as plain loops: the contract smi_lists_regroup and
`sonar_amd.index.regroup_lists` are tested against.

Old storage: ids [slots] (-1: no row), offsets [K + 1], payload [slots, w] bytes, aux [slots] 32-bit words or None.  A slot
survives iff it lies below offsets[K] and its id is >= 0.  New rows: row i goes to list labels[i] (outside [0, K): left out)
with id new_ids[i] (below 0: left out) or id_base + i.  List c of the result holds the survivors of old list c and the new
rows labelled c, each entry with its payload bytes, aux word and id unchanged; the layout is tests/ivf_ref.build's.
"""
import numpy as np

from tests.ivf_ref import ALIGN


def regroup(k, old=None, new=None, id_base=0, a=ALIGN):
    """old: None or (ids, offsets, payload uint8 [slots, w], aux uint32 [slots] | None); new: None or (labels, new_ids | None,
    payload uint8 [>= n, w], aux uint32 [>= n] | None).  Returns (offsets int64 [k + 1], sizes int64 [k], lists): lists[c] is
    the list of (id, payload bytes, aux word or 0) of list c, in the order survivors by slot, then new rows by row."""
    lists = [[] for _ in range(k)]
    if old is not None:
        ids, offsets, payload, aux = old
        for c in range(k):
            for slot in range(int(offsets[c]), int(offsets[c + 1])):
                if int(ids[slot]) >= 0:
                    lists[c].append((int(ids[slot]), bytes(payload[slot]), int(aux[slot]) if aux is not None else 0))
    if new is not None:
        labels, new_ids, payload, aux = new
        for i, c in enumerate(labels):
            rid = int(new_ids[i]) if new_ids is not None else id_base + i
            if 0 <= int(c) < k and rid >= 0:
                lists[int(c)].append((rid, bytes(payload[i]), int(aux[i]) if aux is not None else 0))
    offsets = [0]
    for members in lists:
        offsets.append(offsets[-1] + (len(members) + a - 1) // a * a)
    return np.array(offsets, dtype=np.int64), np.array([len(m) for m in lists], dtype=np.int64), lists


def storage_lists(k, ids, offsets, sizes, payload, aux, width):
    """A storage as `regroup` returns its lists, sorted by id -- after checking its layout: every list starts at a multiple of
    ALIGN, its rows are its first sizes[c] slots... in ANY order, so: sizes[c] slots of the list hold a row, the others are pads
    (id -1, zero payload, aux 0), and ids are -1 from offsets[k] on."""
    lists = []
    assert int(offsets[0]) == 0
    for c in range(k):
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        assert lo % ALIGN == 0 and hi - lo == (int(sizes[c]) + ALIGN - 1) // ALIGN * ALIGN, (c, lo, hi, int(sizes[c]))
        members = []
        for slot in range(lo, hi):
            if int(ids[slot]) >= 0:
                members.append((int(ids[slot]), bytes(payload[slot]), int(aux[slot]) if aux is not None else 0))
            else:
                assert int(ids[slot]) == -1 and bytes(payload[slot]) == bytes(width), slot
                assert aux is None or int(aux[slot]) == 0, slot
        assert len(members) == int(sizes[c]), (c, len(members), int(sizes[c]))
        lists.append(sorted(members))
    assert (np.asarray(ids[int(offsets[k]):]) == -1).all()
    return lists
