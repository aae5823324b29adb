// What the Swin window kernels (swin_attn.hip, swin_block.hip) share: the window geometry that is built, and the SW-MSA regions.
#pragma once

constexpr int WS = 7, WT = 49, HD = 32;   // window side, tokens per window, head dimension

// SW-MSA region (0..8) of the token at (sy, sx) of the shifted, padded Hp x Wp grid: {0: s < L - 7, 1: s < L - shift, 2: rest} per axis.
// Tokens of one window attend to each other only within a region (swin_transformer.py:369-387); only the last window row / column mixes regions.
__device__ __forceinline__ int swin_region(int sy, int sx, int Hp, int Wp, int shift) {
  const int ry = sy < Hp - WS ? 0 : (sy < Hp - shift ? 1 : 2);
  const int rx = sx < Wp - WS ? 0 : (sx < Wp - shift ? 1 : 2);
  return ry * 3 + rx;
}
