// ycc.h - the JFIF luma of an 8-bit RGB pixel in 16.16 fixed point, stated once: the baseline JPEG encoder's Y plane
// (jpegenc.hip) and the planes of the inter-frame tracker (track.hip) are this expression.
#pragma once

__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
