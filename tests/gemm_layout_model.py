"""Python model of gemm_layout_kernel's LDS addressing (video-3d-llm_amd/csrc/gemm.hip): where the LDS-DMA staging puts every
(row, k) of an operand tile, and what the row read (ds_read_b128) and the transposed read (two ds_read_b64_tr_b16) hand to every lane.

Not a conftest: tests/test_gemm_layouts_host.py imports it.  The formulas below are the kernel's, written with the same names
(pw, w4, krow, ch, trb, trc, row0 / row1); the checks on them are in the test module.

Geometry.  Tile form `big` False: 128 x 128 x 64, 4 waves (wm, wn) = (w / 2, w % 2) of 64 x 64; True: 256 x 256 x 64, 8 waves
(w / 4, w % 4) of 128 x 64.  An operand tile is NP = 1 / 2 panels of 16 KiB, a stage is [A tile | B tile], the ring two stages:
  K-contiguous panel  [128 rows][64 k], 128-byte rows, 16-byte chunk c of row r in slot c ^ ((r >> 1) & 7)
  k-major panel       [64 k][128 rows], 256-byte rows, chunk c of k-row r in slot c ^ (((r & 3) << 2) | ((r >> 2) & 3))
A DMA instruction writes wave-uniform base + 16 * lane (1 KiB); the swizzle is in the per-lane SOURCE address.

Hardware rules used (public gfx950 documentation):
  ds_read_b64_tr_b16: per 16 consecutive lanes, lane 4q + p supplies the address of row q, columns 4p .. 4p + 3 of a 4 x 16 block of
  16-bit elements; lane i receives column i, row q in its element q.
  16 x 16 x 32 MFMA operand: lane l holds row l & 15, k = 8 (l >> 4) + j in element j.
  Banks: byte address a is bank (a / 4) % 64 for both reads; lanes conflict inside one group only - the two 32-lane halves for
  ds_read_b64_tr_b16, four 16-lane groups for ds_read_b128; equal addresses broadcast.
"""
LP_BYTES = 16384
B128_GROUPS = ([0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31])
B128_GROUPS = B128_GROUPS + tuple([l + 32 for l in g] for g in B128_GROUPS)
HALVES = (list(range(32)), list(range(32, 64)))


def geometry(big):
    return dict(waves=8 if big else 4, np=2 if big else 1, nwn=4 if big else 2, mt=8 if big else 4, tile=(2 if big else 1) * LP_BYTES)


def stage_image(big, kmajor):
    """One operand tile after a K-step's staging: {byte offset in the tile (even): (row in the tile, k in the K-step)}, built
    from every wave's four DMA pieces.  Each lane moves 16 bytes = 8 consecutive elements along the operand's contiguous dimension."""
    g = geometry(big)
    image = {}
    for wave in range(g["waves"]):
        pw, w4 = wave >> 2, wave & 3
        for i in range(4):
            base = pw * LP_BYTES + w4 * 4096 + i * 1024
            for lane in range(64):
                dst = base + 16 * lane                                   # lane-linear destination
                for e in range(8):
                    if kmajor:
                        krow = w4 * 16 + 4 * i + (lane >> 4)
                        ch = (lane & 15) ^ (((lane >> 4) << 2) | i)
                        src = (pw * 128 + ch * 8 + e, krow)
                    else:
                        row = pw * 128 + w4 * 32 + i * 8 + (lane >> 3)
                        chunk = (lane & 7) ^ ((row >> 1) & 7)
                        src = (row, chunk * 8 + e)
                    assert dst + 2 * e not in image
                    image[dst + 2 * e] = src
    assert len(image) == g["tile"] // 2
    return image


def wave_origin(big, operand, wave):
    """First tile row of the wave's fragments of operand 'A' (m) / 'B' (n)."""
    g = geometry(big)
    wm, wn = wave // g["nwn"], wave % g["nwn"]
    return wm * g["mt"] * 16 if operand == "A" else wn * 64


def read_addresses(big, operand, kmajor, wave, frag, ks):
    """Byte addresses (inside the operand tile) of the LDS instructions that fetch fragment `frag` (16 rows from wave_origin + 16 frag)
    of k-half ks: [[64 lane addresses]] for the row read, two such lists for the transposed read."""
    g = geometry(big)
    wm, wn = wave // g["nwn"], wave % g["nwn"]
    out = []
    if not kmajor:
        wave_base = wave_origin(big, operand, wave) * 128
        lanes = []
        for lane in range(64):
            sw, frow = (lane >> 1) & 7, (lane & 15) * 128
            lanes.append(wave_base + frow + (((4 * ks + (lane >> 4)) ^ sw) << 4) + 2048 * frag)
        return [lanes]
    for e in range(2):
        lanes = []
        for lane in range(64):
            gq, q, pp = lane >> 4, (lane >> 2) & 3, lane & 3
            trb = 256 * (8 * gq + q) + 8 * (pp & 1)
            trc = 16 * ((pp >> 1) ^ ((q << 2) | (2 * (gq & 1))))
            if operand == "A":
                r0, r1 = (wm * LP_BYTES if big else 0) + trb, trc ^ (0 if big else 128 * wm)
            else:
                r0, r1 = (wn >> 1) * LP_BYTES + trb, trc ^ (128 * (wn & 1))
            lanes.append(r0 + (r1 ^ (32 * frag + 16 * e)) + 8192 * ks + 1024 * e)
        out.append(lanes)
    return out


def fragment(big, operand, kmajor, wave, frag, ks, image, ring=0):
    """What the reads deliver: {(lane, element j): (tile row, k)} looked up in a staged image whose keys start at byte `ring`
    (the tile's place in the ring: the kernel adds it to every address alike)."""
    got = {}
    reads = read_addresses(big, operand, kmajor, wave, frag, ks)
    if not kmajor:
        for lane, a in enumerate(reads[0]):
            for j in range(8):
                got[(lane, j)] = image[a + ring + 2 * j]
        return got
    for e, lanes in enumerate(reads):
        for grp in range(4):
            for i in range(16):                                          # receiving lane: column i of the block
                for q in range(4):                                       # element q = row q, whose address lane 4q + (i >> 2) supplied
                    a = lanes[16 * grp + 4 * q + (i >> 2)] + ring
                    got[(16 * grp + i, 4 * e + q)] = image[a + 2 * (i & 3)]
    return got


def expected_fragment(big, operand, wave, frag, ks):
    """The 16 x 16 x 32 operand map: lane l, element j <- (row origin + 16 frag + (l & 15), k = 32 ks + 8 (l >> 4) + j)."""
    r0 = wave_origin(big, operand, wave) + 16 * frag
    return {(lane, j): (r0 + (lane & 15), 32 * ks + 8 * (lane >> 4) + j) for lane in range(64) for j in range(8)}


def conflict_degree(lanes, width, groups):
    """Worst number of DISTINCT addresses on one bank inside one lane group (1 = conflict-free), by the bank rule (a / 4) % 64."""
    worst = 1
    for grp in groups:
        banks = {}
        for lane in grp:
            for b in range(width // 4):
                banks.setdefault((lanes[lane] // 4 + b) % 64, set()).add(lanes[lane])
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def read_conflicts(big, operand, kmajor):
    """Worst conflict degree over every wave, fragment, k-half and instruction of an operand's reads."""
    g = geometry(big)
    nfrag = g["mt"] if operand == "A" else 4
    worst = 1
    for wave in range(g["waves"]):
        for frag in range(nfrag):
            for ks in range(2):
                for lanes in read_addresses(big, operand, kmajor, wave, frag, ks):
                    worst = max(worst, conflict_degree(lanes, 8, HALVES) if kmajor else conflict_degree(lanes, 16, B128_GROUPS))
    return worst
