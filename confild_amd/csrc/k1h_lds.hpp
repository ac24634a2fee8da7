// K1h on v_mfma_f32_16x16x32_f16 (conv_x.hip, conv_h_kernel<..., SHAPE = 16>): the
// LDS address functions of the halo and of the weight ring, as plain constexpr
// functions of integers so that a host program can evaluate them
// (tests/test_k1h_lds_host.py checks every ds_read_b128 and staging store of the
// kernel for bank conflicts and for staying inside its plane).
//
// A halo or ring row is one pixel's (one output channel's) 32 f16 = four 16-B
// chunks.  Lane roles as K1p's: a fragment read takes row lane % 16 of a 16-row
// block, chunk lane / 16 (channels 8g .. 8g + 7).  Chunk c of row r sits in slot
// (c + 2 * bit 2 of r) & 3 (lds_swz_bf's rule, unet_kernels.hip): the rotation
// depends on r / 4 alone and has period 2 in it, so any 16 CONSECUTIVE rows --
// whatever the first one, which the tap shifts -- put each of ds_read_b128's
// four 16-lane groups on the 16 slots of the 256-B bank row once.
//
// The halo's LDS row stride is the tile's TW + 2 columns padded to a multiple of
// 8 pixels.  Moving by a tile row, a kernel row (ty) or a 16-pixel block then
// moves the address by a multiple of 512 B and leaves the rotation alone: of a
// wave's 4 row blocks x 9 taps only the three column shifts tx need an address
// register, the rest are instruction offsets.  A 16-pixel block never spans two
// tile rows (TW >= 16), so the 32x32x16 form's TW = 16 row term is not needed.
// The pad columns are neither staged nor read.
#pragma once

namespace cfd {

// chunk slot rotation; swz = false is the plain layout (the test's negative control)
constexpr int k1h_swz(int row, int chunk, bool swz = true) {
    return row * 64 + ((chunk + (swz ? 2 * ((row >> 2) & 1) : 0)) & 3) * 16;
}
// halo row stride in LDS, pixels
constexpr int k1h_hws(int tw) { return (tw + 2 + 7) / 8 * 8; }
// halo pixels in LDS (bytes of one f16 plane: 64 per pixel)
constexpr int k1h_npx(int bm, int tw) { return (bm / tw + 2) * k1h_hws(tw); }
// staged halo pixels: the dense (TR + 2) x (TW + 2) list, 8 threads per pixel
constexpr int k1h_npx_staged(int bm, int tw) { return (bm / tw + 2) * (tw + 2); }
// LDS pixel of staged pixel hp
constexpr int k1h_stage_px(int tw, int hp) { return (hp / (tw + 2)) * k1h_hws(tw) + hp % (tw + 2); }
// byte offset of the 8-B staging store of channel quad kq (0..7) of staged pixel hp
constexpr int k1h_stage_off(int tw, int hp, int kq, bool swz = true) {
    return k1h_swz(k1h_stage_px(tw, hp), kq >> 1, swz) + (kq & 1) * 8;
}
// A fragment of wave row wm (64 tile pixels each), lane (li, g), column shift tx:
// the address register (row block 0, kernel row 0)
constexpr int k1h_a_base(int tw, int wm, int li, int g, int tx, bool swz = true) {
    return k1h_swz((wm * 64 / tw) * k1h_hws(tw) + li + tx, g, swz);
}
// ... and the instruction offset of row block i (16 tile pixels each) at kernel row ty
constexpr int k1h_a_imm(int tw, int i, int ty) { return ((16 * i / tw + ty) * k1h_hws(tw) + 16 * i % tw) * 64; }
// B fragment of wave column wn (64 output channels each): address register of
// block 0, and the instruction offset of block j
constexpr int k1h_b_base(int wn, int li, int g, bool swz = true) { return k1h_swz(wn * 64 + li, g, swz); }
constexpr int k1h_b_imm(int j) { return 16 * j * 64; }
// the 16-B staging store of chunk bq of weight row `row`
constexpr int k1h_wstage_off(int row, int bq, bool swz = true) { return k1h_swz(row, bq, swz); }
// epilogue stage (floats): pixel row of BN channels, 16-channel groups XORed with
// (row / 4) & 3 -- the four lane groups of an accumulator (rows 4g .. 4g + 3 of one
// channel per lane) then store to different banks, and float4 pieces stay whole
constexpr int k1h_epi(int bn, int row, int col) { return row * bn + (col ^ (((row >> 2) & 3) << 4)); }

}  // namespace cfd
