// grok_amd/csrc/decode_internal.h -- what the decode path's units share: decode_blocks.hip (tables and block decoders), decode.hip
// (a call from table to pixels) and decode_sequence.hip (frames in flight on internal contexts).
#pragma once
#include "context.h"
#include "decode_plan.h"

#pragma GCC visibility push(hidden)
// ---- decode_blocks.hip ----
// The pinned tables of this call with the caller's rows in them (room for the launch lists behind the rows); the set's last upload
// has been waited for (two calls ago: long done).  nblocks counts the rows of the context's geometry (a reduced one: fewer than
// the caller's table holds)
int stage_table(grk_amd_ctx* c, const grk_amd_coded_block* table, uint64_t nblocks, grk_amd_ctx::DecUpload** out);
// the staged rows' blocks into d_mallat.  h16: int16 planes; split: K5b in two parts for a call that goes on with the inverse transform
int run_ht_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat,
                  bool h16 = false, bool split = false);
int run_t1_decode(grk_amd_ctx* c, uint32_t ntiles, grk_amd_ctx::DecUpload* up, const void* d_coded, uint64_t coded_bytes, void* d_mallat);
// what the block decoders left in the status word (synchronises the context's stream)
int check_decode_status(grk_amd_ctx* c);
// ---- decode.hip ----
// one decode call on context c: win != nullptr a region decode, force32 the exact path after GRK_AMD_ERR_RANGE
int decode_impl(grk_amd_ctx* c, const grk_amd_tile_params* p, uint32_t ntiles, const grk_amd_coded_block* table, const void* coded,
                uint64_t coded_bytes, int coded_on_device, void* pixels, int pixels_on_device, const Rect* win, bool force32 = false);
#pragma GCC visibility pop
