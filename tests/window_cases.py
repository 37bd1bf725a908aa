"""What the window decode tests of both stream versions share: the fixed, seeded window list of an image and the sentinel discipline -- the output buffer is filled
with a sentinel, has a stride larger than the window, and after the call the window must equal the crop of the full decode AND every other element must still hold
the sentinel."""
import numpy as np

SENTINEL = 0x5A5A5A5A
ERRORS = {"InvalidParameter": 101, "ArgumentNull": 102, "OutOfBounds": 103}  # limg_hip_result (include/limg_hip.h)


def windows(W, H, seed=1):
    """(x, y, w, h) list: the whole image, 1 x 1 at the four corners, a block-aligned window, one with all four edges unaligned, a single row and a single column through
    the whole image, on images that are not in whole blocks one that ends in the partial edge blocks, and three seeded ones."""
    rng = np.random.RandomState(seed * 7919 + W * 31 + H)
    out = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
    ax, ay = (8 if W >= 16 else 0), (8 if H >= 16 else 0)
    out.append((ax, ay, max(8, min(32, (W - ax) // 8 * 8)) if W - ax >= 8 else W - ax, max(8, min(16, (H - ay) // 8 * 8)) if H - ay >= 8 else H - ay))  # block-aligned
    if W >= 4 and H >= 4:  # all four edges off the block grid (and off the 16-byte grid)
        for _ in range(1000):
            x, y = int(rng.randint(1, W - 2)), int(rng.randint(1, H - 2))
            w, h = int(rng.randint(1, W - x)), int(rng.randint(1, H - y))
            if x % 8 and y % 8 and (x + w) % 8 and (y + h) % 8 and x + w < W and y + h < H:
                out.append((x, y, w, h))
                break
    out.append((0, int(rng.randint(0, H)), W, 1))  # a single row
    out.append((int(rng.randint(0, W)), 0, 1, H))  # a single column
    if W % 8 or H % 8:  # ends in the partial edge blocks
        w, h = min(11, W), min(13, H)
        out.append((W - w, H - h, w, h))
    for _ in range(3):
        x, y = int(rng.randint(0, W)), int(rng.randint(0, H))
        out.append((x, y, int(rng.randint(1, W - x + 1)), int(rng.randint(1, H - y + 1))))
    assert all(w >= 1 and h >= 1 and x + w <= W and y + h <= H for x, y, w, h in out), out
    return out


def host_window(decode, stream, want, win):
    """`decode(stream, x, y, w, h, out=view)` into the middle of a sentinel-filled array: the window equals the crop of `want`, everything else holds the sentinel"""
    x, y, w, h = win
    buf = np.full((h + 3, w + 7), SENTINEL, dtype=np.uint32)
    decode(stream, x, y, w, h, out=buf[1:1 + h, 2:2 + w])
    exp = np.full_like(buf, SENTINEL)
    exp[1:1 + h, 2:2 + w] = want[y:y + h, x:x + w]
    assert np.array_equal(buf, exp), (win, np.argwhere(buf != exp)[:6].tolist())


def device_window(decode, dstream, nbytes, W, H, want, win, unaligned):
    """The device entry into a sentinel-filled flat buffer.  unaligned: pOut 4 bytes off a 16-byte boundary and an odd stride, so every piece leaves as dword stores;
    otherwise pOut 16-byte aligned and the stride a multiple of 4 (windows with x % 4 == 0 then take the 16-byte stores).  want: numpy uint32 or torch int32 (H, W)."""
    import torch
    x, y, w, h = win
    stride = (w + 5) | 1 if unaligned else (w + 8) // 4 * 4
    off = 4 * stride + (1 if unaligned else 0) + (0 if unaligned else (-4 * stride) % 4)
    flat = torch.full((off + (h + 2) * stride + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    assert (flat.data_ptr() + 4 * off) % 16 == (4 if unaligned else 0)
    decode(dstream, nbytes, W, H, x, y, w, h, out=flat[off:], out_stride=stride)
    torch.cuda.synchronize()
    if isinstance(want, np.ndarray):
        want = torch.from_numpy(want.view(np.int32)).cuda()
    exp = torch.full_like(flat, SENTINEL)
    exp[off:off + h * stride].view(h, stride)[:, :w] = want[y:y + h, x:x + w]
    assert torch.equal(flat, exp), (win, unaligned, torch.nonzero(flat != exp)[:6].ravel().tolist())


def blocks_of(win):
    """the window's block range: bx0, by0, bx1, by1 (inclusive)"""
    x, y, w, h = win
    return x // 8, y // 8, (x + w - 1) // 8, (y + h - 1) // 8
