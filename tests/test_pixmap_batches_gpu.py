"""More descriptors than a grid has rows in y: a call of 65540 frames of 4 x 1 through the posterize and the colormap
stage is cut into launches of 65535 and 5, and the colormap's table crosses the cut on the device.  Sources are shared,
every destination is a 32-byte slot of one tensor -- 16 guard bytes in front of the even ones (16-byte stores), 8 in
front of the odd ones (dword stores)."""
import numpy as np
import pytest

import _pixmap_ref as R
import ntscsim

pytestmark = pytest.mark.gpu

N, SLOT, K = 65540, 32, 8


def slots(torch, seed):
    init = np.random.RandomState(seed).randint(0, 256, size=(N, SLOT), dtype=np.uint8)
    big = torch.from_numpy(init).cuda()
    flat = big.view(-1)
    off = [16 if i % 2 == 0 else 8 for i in range(N)]
    views = [torch.as_strided(flat, (1, 4, 4), (16, 4, 1), i * SLOT + off[i]) for i in range(N)]
    return init, big, np.array(off), views


def check(init, big, off, content):
    """content[i]: the 16 bytes descriptor i must have written"""
    want = init.copy()
    for o in (8, 16):
        rows = np.nonzero(off == o)[0]
        want[rows, o:o + 16] = content[rows]
    got = big.cpu().numpy()
    bad = (got != want).any(axis=1)
    assert not bad.any(), "%d destinations differ, the first is %d" % (int(bad.sum()), int(np.argmax(bad)))


def test_posterize_more_than_65535_descriptors():
    import torch
    hsrc = [np.random.RandomState(6000 + k).randint(0, 256, size=(1, 4, 4)).astype(np.uint8) for k in range(K)]
    dsrc = [torch.from_numpy(s).cuda() for s in hsrc]
    init, big, off, views = slots(torch, 6100)
    post = ntscsim.Posterizer(sum((["-i", "x", "-threshhold", str(t)] for t in range(9)), []), width=4, height=1)
    try:
        post.frames([(views[i], dsrc[i % K], i % 9) for i in range(N)])
        post.sync()
        assert post.last_kernels() == ["k_post_frames"] * 2
        table = np.stack([[R.posterize(hsrc[k], t).reshape(16) for t in range(9)] for k in range(K)])
        idx = np.arange(N)
        check(init, big, off, table[idx % K, idx % 9])
    finally:
        post.close()


def test_colormap_more_than_65535_descriptors_and_the_table_across_the_cut():
    import torch
    rng = np.random.RandomState(6200)
    hsrc = [rng.randint(0, 256, size=(1, 4, 4)).astype(np.uint8) for _ in range(K)]
    dsrc = [torch.from_numpy(s).cuda() for s in hsrc]
    hmap = {5: rng.randint(0, 256, size=(1, 4, 4)).astype(np.uint8), 65530: rng.randint(0, 256, size=(1, 4, 4)).astype(np.uint8)}
    dmap = {i: torch.from_numpy(m).cuda() for i, m in hmap.items()}
    init, big, off, views = slots(torch, 6300)
    cm = ntscsim.ColorMapper(width=4, height=1)
    try:
        cm.frames([(views[i], dsrc[i % K], dmap.get(i)) for i in range(N)])
        cm.sync()
        # the maps are in the first launch; the second has none and goes by the table the first left behind
        assert cm.last_kernels() == ["k_cmap_frames", "k_cmap_take", "k_cmap_frames"]
        tables = [R.identity_table(), R.take(hmap[5]), R.take(hmap[65530])]
        out = np.stack([[R.apply(hsrc[k], t).reshape(16) for t in tables] for k in range(K)])
        idx = np.arange(N)
        which = (idx >= 5).astype(int) + (idx >= 65530).astype(int)
        assert which[65535:].tolist() == [2] * 5 and (out[:, 2] != out[:, 1]).any()
        check(init, big, off, out[idx % K, which])
        assert (cm.table == tables[2]).all()
    finally:
        cm.close()
