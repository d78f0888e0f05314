"""Host-side checks of the sub-pixel weight gradient (jg_wgrad_args.x_mode 2, csrc/wgrad_halo.hip wgrad3x3_subpixel_kernel): the
(phase, tap) -> halo-offset table and the 16 -> 9 combination, written as data the way the kernel codes them, reproduce autograd in
float64; the parity-plane LDS-DMA source index and the LDS position it lands on are a bijection for one tile, and the fragment reader
finds every (pixel, channel block) where the DMA put it.  No GPU."""
import torch
import torch.nn.functional as F

TL, HW_ = 4, 18                       # low-resolution tile rows, halo width
HALO_CH = (TL + 2) * HW_ * 8          # 16-byte chunks of the halo
PL_CH = TL * 16 * 8                   # chunks of one parity plane (= the 512 threads of a workgroup: one DMA round per plane)


def acc_index(py, px, a, b):
    """the kernel's accumulator numbering: acc[(grp & 3) * 4 + tap], grp & 3 = py * 2 + px, tap = a * 2 + b"""
    return ((py * 2 + px) * 2 + a) * 2 + b


def halo_offset(step):
    """load_fb: (row, column) offset into the zero-padded halo of step = (sub * 4 + ph) * 4 + a * 2 + b, without the 2 * sub rows"""
    ph, a, b = (step >> 2) & 3, (step >> 1) & 1, step & 1
    return a + (ph >> 1), b + (ph & 1)


def combination(r, s):
    """the epilogue: the four accumulators summed into dw[r][s], in the kernel's order"""
    a0, a1 = (0 if r == 0 else 1), (1 if r == 2 else 0)          # tap of phase 0 / phase 1 on the vertical axis
    b0, b1 = (0 if s == 0 else 1), (1 if s == 2 else 0)
    return [acc_index(0, 0, a0, b0), acc_index(0, 1, a0, b1), acc_index(1, 0, a1, b0), acc_index(1, 1, a1, b1)]


def test_tables_agree_with_the_fold_sets():
    sets = {(0, 0): [0], (0, 1): [1, 2], (1, 0): [0, 1], (1, 1): [2]}     # (phase, tap) -> 3x3 taps, per axis
    for r in range(3):
        for s in range(3):
            want = sorted(acc_index(py, px, a, b) for py in (0, 1) for px in (0, 1) for a in (0, 1) for b in (0, 1)
                          if r in sets[(py, a)] and s in sets[(px, b)])
            assert sorted(combination(r, s)) == want and len(want) == 4
    offs = {halo_offset(step) for step in range(16)}
    assert offs == {(i, j) for i in range(3) for j in range(3)}          # the 9 offsets of the ordinary 18-wide halo
    for step in range(16):
        ph, a, b = step >> 2, (step >> 1) & 1, step & 1
        assert halo_offset(step) == (a + (ph >> 1), b + (ph & 1)) and acc_index(ph >> 1, ph & 1, a, b) == step


def test_tables_reproduce_autograd_in_float64():
    B, Hl, Wl, Ci, Co = 2, 5, 6, 8, 4
    g = torch.Generator().manual_seed(3)
    h = torch.randn((B, Ci, Hl, Wl), generator=g, dtype=torch.float64)
    dO = torch.randn((B, Co, 2 * Hl, 2 * Wl), generator=g, dtype=torch.float64)
    w = torch.zeros((Co, Ci, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), w, None, padding=1).backward(dO)
    hpad = F.pad(h, (1, 1, 1, 1))
    acc = [None] * 16
    for step in range(16):
        ph = step >> 2
        py, px = ph >> 1, ph & 1
        oy, ox = halo_offset(step)
        plane = dO[:, :, py::2, px::2]                                           # [B, Co, Hl, Wl]
        win = hpad[:, :, oy:oy + Hl, ox:ox + Wl]                                 # [B, Ci, Hl, Wl]
        acc[step] = torch.einsum("bohw,bihw->oi", plane, win)
    for r in range(3):
        for s in range(3):
            i0, i1, i2, i3 = combination(r, s)
            got = (acc[i0] + acc[i1]) + (acc[i2] + acc[i3])
            assert torch.allclose(got, w.grad[:, :, r, s], rtol=1e-12, atol=1e-12), (r, s)


def f4(c):      # csrc/lds_dma.h f4: 2-bit block swizzle of a 128-byte pixel row by pixel column
    return ((c >> 1) & 1) | (((c >> 3) & 1) << 1)


def test_parity_plane_dma_is_a_bijection_and_the_reader_finds_it():
    W, ld = 64, 72                                 # upsampled row length (pixels) and pixel stride (elements) of dO
    src_seen, lds = set(), {}
    for pl in range(4):
        py, px = pl >> 1, pl & 1
        for tid in range(512):
            # issue_tile / d_rel: thread tid brings chunk cpos of low-resolution tile pixel (ty, xx) of plane (py, px)
            p, cpos = tid >> 3, tid & 7
            ty, xx = p >> 4, p & 15
            chunk = ((((cpos >> 1) ^ f4(xx)) << 1) | (cpos & 1))
            src = ((2 * ty * W + 2 * xx) + (py * W + px)) * ld + chunk * 8     # element offset from the tile's first dO element
            pos = HALO_CH + pl * PL_CH + tid                                    # LDS chunk position (lane-linear DMA)
            row, col = divmod(src // ld, W)
            assert src % ld == chunk * 8 and 0 <= row < 2 * TL and 0 <= col < 32
            assert (row & 1, col & 1) == (py, px) and (row >> 1, col >> 1) == (ty, xx)
            src_seen.add((row, col, chunk))
            assert pos not in lds
            lds[pos] = (pl, ty, xx, chunk)
    assert len(src_seen) == 2 * TL * 32 * 8 and sorted(lds) == list(range(HALO_CH, HALO_CH + 4 * PL_CH))
    # the fragment reader (abase + plane offset + sub-step offset): lane (g, i16) of wave row wm, fragment i, half rd, addresses the four
    # channels (i16 & 3) * 4 .. + 3 of channel block cb = wm * 2 + i at plane pixel (2 sub + trow, xq)
    for pl in range(4):
        for sub in range(TL // 2):
            for wm in range(2):
                for i in range(2):
                    for lane in range(64):
                        i16, g = lane & 15, lane >> 4
                        trow = g >> 1
                        for rd in range(2):
                            xq = (g & 1) * 8 + rd * 4 + (i16 >> 2)
                            cb = wm * 2 + i
                            byte = HALO_CH * 16 + (trow * 16 + xq) * 128 + ((cb ^ f4(xq)) << 5) + (i16 & 3) * 8 + pl * PL_CH * 16 + sub * 32 * 128
                            assert lds[byte >> 4] == (pl, 2 * sub + trow, xq, cb * 2 + ((i16 & 3) >> 1))
