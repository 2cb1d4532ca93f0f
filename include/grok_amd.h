/* include/grok_amd.h -- the C-ABI of the MI355X tile processor (libgrok_amd.so).
 *
 * This is the thin C layer SURVEY.md §8(b) asks for underneath the Grok plugin entry points:
 * plain pointers and sizes only (no torch / C++ types), one opaque context per GPU.
 * The plugin shim (libgrokj2k_plugin.so, include/grk_plugin_abi.h) wraps these calls into the
 * grk_plugin_* protocol; bench.py and the parity tests call them through ctypes.
 *
 * Every entry point names the reference interface it replaces (paths relative to the Grok
 * 8.0.2 tree, src/lib/jp2/...):
 *
 *   grk_amd_encode_tiles        TileProcessor::do_compress()  tile/TileProcessor.cpp:665-699
 *                               = dc_level_shift_encode :922, mct_encode :945, dwt_encode :977,
 *                                 t1_encode :992 (T1HT::compress, t1/t1_ht/T1HT.cpp:102-128)
 *   grk_amd_stage_ingest_mct    TileProcessor.cpp:1166-1216 + :922-944 + mct::compress_rev/irrev
 *                               (point_transform/mct.cpp:48-105, :469-554)
 *   grk_amd_stage_dwt_fwd       WaveletFwdImpl::compress (transform/WaveletFwd.cpp:612-620)
 *   grk_amd_stage_ht_encode     T1CompressScheduler::scheduleCompress (t1/T1CompressScheduler.cpp:33-90)
 *                               + ojph_encode_codeblock (t1/t1_ht/coding/ojph_block_encoder.cpp:463)
 *   grk_amd_tile_layout         TileComponent::init geometry (tile/TileComponent.cpp:69-170),
 *                               Quantizer::setBandStepSizeAndBps (codestream/Quantizer.cpp:26-66),
 *                               param_qcd::set_rev_quant/set_irrev_quant (codestream/HTParams.cpp:248-312)
 *   grk_amd_write_codestream    CodeStreamCompress main header + tile parts + T2 packets, restricted
 *                               to 1 layer / LRCP / 1 precinct per resolution
 *                               (codestream/CodeStreamCompress.cpp:722-753, t2/T2Compress.cpp:123-333)
 *
 * Error convention (mirrors the plugin boundary, grok.h:1781): 0 = success, negative = failure /
 * "not handled" so that the host can fall back to its CPU path.  No exceptions cross this ABI.
 */
#ifndef GROK_AMD_H
#define GROK_AMD_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRK_AMD_OK                0
#define GRK_AMD_ERR_NO_DEVICE    -1   /* no HIP device / HIP runtime failure           */
#define GRK_AMD_ERR_UNSUPPORTED  -2   /* parameter combination outside the hot path     */
#define GRK_AMD_ERR_INVALID      -3   /* bad argument                                   */
#define GRK_AMD_ERR_NOMEM        -4
#define GRK_AMD_ERR_OVERFLOW     -5   /* coded data did not fit the arena               */
#define GRK_AMD_ERR_RANGE        -6   /* decode: a value left the 16-bit planes (see grk_amd_set_decode_planes16) */

#define GRK_AMD_MAX_LEVELS 10

typedef struct grk_amd_ctx grk_amd_ctx;      /* one per process per GPU */

/* What the hot path needs out of grk_cparameters / grk_image (grok.h:451-573, :866-929). */
typedef struct grk_amd_tile_params {
    uint32_t tile_w, tile_h;     /* tile-component size (dx=dy=1)                                 */
    uint16_t num_comps;          /* 1..4 ; MCT needs >=3                                        */
    uint8_t  prec;               /* bits per sample, 1..16                                      */
    uint8_t  sgnd;               /* signed samples (DC shift 0)                                 */
    uint8_t  irreversible;       /* 0: RCT + 5/3 (lossless)   1: ICT + 9/7 + dead-zone quantiser*/
    uint8_t  mct;                /* tcp_mct: component transform on components 0..2             */
    uint8_t  num_levels;         /* numresolution - 1                                           */
    uint8_t  cblk_w_exp;         /* log2 code-block width  (6)                                  */
    uint8_t  cblk_h_exp;         /* log2 code-block height (6)                                  */
    uint8_t  reserved[3];        /* [0]: decode only -- 1 = the blocks are Part-1 (EBCOT/MQ) instead of HT;
                                    then missing_msbs of a table row carries numbps | numpasses << 8
                                    (block bit-planes coded, coding passes in total)
                                    [1]: Part-1 decode -- the COD code-block style bits as the reference
                                    names them (grok.h GRK_CBLKSTY_*): LAZY 0x01, RESET 0x02, TERMALL 0x04,
                                    VSC 0x08, PTERM 0x10, SEGSYM 0x20                                 */
    uint32_t tile_x0, tile_y0;   /* the tile's origin on the canonical grid (grk_image x0/y0, tile grid: the tile's x0/y0 as
                                    TileProcessor::init computes it).  0, 0 for an image at the origin with one tile; any
                                    other value changes the sub-band sizes, the code-block partition and, where a
                                    resolution starts on an odd coordinate, the lifting variant (WaveletFwd.cpp:884-905) */
    uint8_t  precinct_exp[12];   /* [r] = PPx | PPy << 4 of resolution r (0 = coarsest), as the COD marker carries them
                                    (grk_compress -c; TileComponentCodingParams::precinctWidthExp / HeightExp); 0 = not set
                                    = 15 | 15 << 4: one precinct per resolution (so PPx = PPy = 0, legal for r = 0 only, cannot
                                    be asked for).  Precincts cut the code-block partition
                                    (code-block exponent <= precinct exponent of the band) and make one packet each, in
                                    any of the five progression orders */
} grk_amd_tile_params;

/* One code-block of the tile, in the reference's enumeration order
 * comp -> resolution -> band -> precinct(1) -> raster (T1CompressScheduler.cpp:44-85). */
typedef struct grk_amd_block {
    uint32_t x0, y0, x1, y1;     /* band coordinates (what grk_plugin_code_block.x0.. carries) */
    uint32_t px, py;             /* origin inside the component's Mallat plane                 */
    uint16_t comp;
    uint8_t  res;                /* 0 = coarsest                                               */
    uint8_t  band;               /* orientation 0 LL, 1 HL, 2 LH, 3 HH                         */
    uint8_t  kmax;               /* band->numbps (= QCD exponent for HT, numgbits 1)           */
    uint8_t  reserved[3];
    float    stepsize;           /* band->stepsize (1.0 reversible)                            */
    uint32_t precinct;           /* index of its precinct in the resolution's precinct grid (raster)  */
} grk_amd_block;

/* Result row per coded block. `offset` is relative to the start of the coded arena. */
typedef struct grk_amd_coded_block {
    uint64_t offset;
    uint32_t length;             /* MagSgn | MEL | VLC bytes of the single HT cleanup pass      */
    uint32_t missing_msbs;       /* band numbps - block numbps: what the decoder needs besides the
                                    bytes (Kmax - 1 for blocks of this encoder, T1HT.cpp:123)    */
} grk_amd_coded_block;

/* ---- lifecycle ---------------------------------------------------------------------------- */
/* plugin_init(grk_plugin_init_info{deviceId,verbose}) -> grk_amd_create (grok.h:1749-1757) */
int  grk_amd_create(int device_id, int verbose, grk_amd_ctx** out);
void grk_amd_destroy(grk_amd_ctx* ctx);
const char* grk_amd_version(void);
/* sha1 over the sources (grok_amd/csrc, include) the library was built from, as __graft_entry__.source_stamp() computes it for a
 * tree: the test suite compares the two, so that a stale prebuilt library cannot pass for the tree it travels with */
const char* grk_amd_source_stamp(void);
const char* grk_amd_last_error(grk_amd_ctx* ctx);
/* use an externally owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream); NULL = own */
int  grk_amd_set_stream(grk_amd_ctx* ctx, void* hip_stream);
/* Pinned (page-locked) host memory for the buffers handed to the host-pointer entry points below (on_device = 0): such a
 * buffer crosses the link in one DMA at the link's rate (~50 GB/s each way on MI355X hosts).  Any other host memory works
 * too -- it is moved through context-owned pinned chunks by a few copy threads, at those threads' memcpy rate.  What the
 * reference would do in grk_plugin_compress's image reader: the plugin's own loader reads files into such memory. */
void* grk_amd_host_alloc(grk_amd_ctx* ctx, uint64_t bytes);
void  grk_amd_host_free(grk_amd_ctx* ctx, void* p);

/* ---- geometry (host only, no GPU needed) ---------------------------------------------------- */
/* Number of code-blocks in one tile (all components). */
int64_t grk_amd_tile_num_blocks(const grk_amd_tile_params* p);
/* Fill `blocks` (capacity cap) in enumeration order; returns count or negative error.
 * Also returns per-band QCD words: reversible -> expn<<3 (u8), irreversible -> (expn<<11)|mant. */
int64_t grk_amd_tile_layout(const grk_amd_tile_params* p, grk_amd_block* blocks, uint64_t cap,
                            uint16_t* qcd_words /* [3*levels+1] or NULL */);
/* precincts of every resolution (counts[r], r = 0 coarsest .. num_levels): the packets a tile-component has per layer */
int grk_amd_tile_precincts(const grk_amd_tile_params* p, uint32_t* counts);
/* int32 elements between consecutive rows / planes of the device working planes */
uint32_t grk_amd_plane_stride(const grk_amd_tile_params* p);
uint64_t grk_amd_plane_elems(const grk_amd_tile_params* p);

/* ---- whole hot path -------------------------------------------------------------------------
 * Encode `num_tiles` tiles of one geometry (grk_amd_same_tile_geometry; the batch is coded with *p) in one batch.  `pixels` holds the tiles back to back,
 * each tile component-major planar, row-major, tightly packed (the default; grk_amd_set_pixel_layout below: interleaved, pitched), ceil(prec/8) bytes per sample,
 * host endian -- the layout grk_compress_tile() takes (TileProcessor.cpp:1177-1213).
 * pixels_on_device != 0: `pixels` is a device pointer (HBM-resident input, what bench.py times).  Lifetime of device pixels: they
 * are read in the order of the context's stream (grk_amd_set_stream) -- whatever the caller queues on that stream behind the call (the
 * next frame's pixels into the same buffer, a stream-ordered free) comes after the read, on every path, pipelined or not
 * (grk_amd_set_pixel_hold below relaxes this for callers that rotate their input buffers).
 *
 * On return the coded bytes of all blocks live in the context's device arena; `table` (host,
 * num_tiles * blocks_per_tile rows, tile-major) describes them.  Pass table == NULL to leave the
 * table on the device as well (fully asynchronous; fetch later with grk_amd_fetch_table). */
int grk_amd_encode_tiles(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                         const void* pixels, int pixels_on_device,
                         grk_amd_coded_block* table, uint64_t* total_bytes);
/* The layout of the pixels an encode reads (default: the one above).  Frames on a GPU are rarely component planes: a camera, a video
 * decoder, an image loader and a channels-last tensor hold H x W x C interleaved samples, rows often carry a pitch and display paths a
 * fourth, unused channel.  Level 0 of the forward transform reads the caller's pixels itself, so a layout is a property of its loads,
 * not a pass of its own: no transposed copy of the frame is made.
 *   interleaved  0: component-major planar (default).  1: pixel-interleaved, sample c of pixel x of a row at x * channels + c
 *   channels     interleaved only: samples per pixel IN MEMORY, num_comps .. 4; 0 = num_comps.  Samples beyond num_comps are skipped
 *                (RGBX, or RGB out of RGBA)
 *   fill         decode, interleaved, channels > num_comps: the value the extra samples receive (opaque alpha); an encode does not read it
 *   row_pitch    bytes between rows, 0 = tight; a multiple of the sample size, at least one tight row
 *   plane_pitch  planar only: bytes between the component planes of a tile, 0 = tight (h * row pitch)
 *   tile_pitch   bytes between the tiles of a batch, 0 = tight
 * A layout does not change which values the pixels have: the coded blocks are those of the same samples in the default layout, bit
 * for bit, and bytes in gaps and skipped channels are never interpreted.  The layout is context state (NULL = default); it cannot
 * be checked before the tile parameters are known, so the calls that use it do that, with grk_amd_pixel_bytes: GRK_AMD_ERR_INVALID and
 * the reason in grk_amd_last_error.  Honoured by grk_amd_encode_tiles (host pixels: the extent grk_amd_pixel_bytes gives goes up as one
 * copy, gaps included; device pixels; pipelined or not), grk_amd_stage_ingest_mct and grk_amd_encode_image (`pixels` = the whole image
 * in this layout, row_pitch the image's, tile_pitch unused).  grk_amd_encode_image_subsampled returns GRK_AMD_ERR_UNSUPPORTED while a
 * layout other than the default is set.  The node API has contexts of its own and the Grok plugin is handed planar int32 by Grok:
 * neither sees this setting.
 * grk_amd_set_decode_pixel_layout: the same for the pixels a decode WRITES -- the last inverse level stores them itself, whole pixels
 * at a time where the alignment allows.  Honoured by grk_amd_decode_tiles (also under grk_amd_set_decode_reduce and in a decode
 * sequence, whose internal contexts inherit it), grk_amd_decode_region (pitches are the window's), grk_amd_stage_egress and
 * grk_amd_decode_image (`pixels` = the whole image in this layout).  Bytes in a row gap, a plane gap or a tile gap are never
 * written -- with host pixels the extent travels both ways for that; the extra samples of interleaved pixels are written with `fill`.
 * Samples of more than 16 bits leave in the default layout only (GRK_AMD_ERR_UNSUPPORTED).
 * Device pixels of 8-bit samples off 4-byte alignment take the separate ingest pass, as in the default layout. */
typedef struct grk_amd_pixel_layout {
    uint8_t  interleaved;
    uint8_t  channels;
    uint16_t fill;
    uint32_t reserved;
    uint64_t row_pitch;
    uint64_t plane_pitch;
    uint64_t tile_pitch;
} grk_amd_pixel_layout;
int grk_amd_set_pixel_layout(grk_amd_ctx* ctx, const grk_amd_pixel_layout* layout);
int grk_amd_set_decode_pixel_layout(grk_amd_ctx* ctx, const grk_amd_pixel_layout* layout);
/* Bytes a buffer of `num_tiles` tiles of w x h samples per component (0 = p->tile_w, p->tile_h) spans in `layout` (NULL = default), from
 * its first sample to the end of its last (interleaved: of its last pixel, skipped channels included); host only.  0 for a layout that is invalid for these parameters: channels below num_comps
 * or above 4, a pitch smaller than what it spans or no multiple of the sample size, plane_pitch together with interleaved. */
uint64_t grk_amd_pixel_bytes(const grk_amd_tile_params* p, const grk_amd_pixel_layout* layout, uint32_t w, uint32_t h, uint32_t num_tiles);
/* Pixel lifetime, relaxed (default off).  Pipelined encodes of small frames run a frame's whole chain on a stream of the context's own
 * (GRK_AMD_FRAME_STREAMS), so keeping the rule above costs a wait of the context's stream per call -- consecutive 512 x 512 frames:
 * 0.057 instead of 0.038 ms per call.  on != 0: the caller PROMISES not to touch a call's device pixels before a stream of its own has
 * passed grk_amd_stream_wait_pixels (or grk_amd_synchronize returned); the wait is then left out.  A ring of input buffers with
 * one grk_amd_stream_wait_pixels before a buffer is refilled is the intended use. */
int grk_amd_set_pixel_hold(grk_amd_ctx* ctx, int on);
/* Pipelined encodes run on three streams (the caller's + two of the context's) whose kernels have to be DISPATCHED side by side; whether
 * they can depends on the hardware queues the runtime gave them, i.e. on the streams the process made before (profiles/r06_hw_queues.txt).
 * Before the first pipelined encode on a given main stream the context probes its streams pairwise (~2 ms, the main stream is
 * synchronised once) and replaces a side stream that has to take turns (GRK_AMD_STREAM_PROBE=0: never).  Returns the number of side
 * streams replaced so far, -1 with the probe off. */
int grk_amd_stream_probe_result(grk_amd_ctx* ctx);
/* the same probe at once (e.g. before a host vets its own streams against the context's) */
int grk_amd_probe_streams(grk_amd_ctx* ctx);
/* ... and for a host's own streams: 1 when kernels of HIP streams a and b are dispatched side by side (both directions), 0 when one waits
 * for the other's grid.  A stream that WAITS for the encoder's results (an exchange's) should pass this against grk_amd_internal_stream(ctx,
 * 0 / 1 / 2) -- the main stream and the two side streams as they are now. */
int grk_amd_streams_side_by_side(grk_amd_ctx* ctx, void* a, void* b);
void* grk_amd_internal_stream(grk_amd_ctx* ctx, int which);
/* Makes `hip_stream` wait until the LATEST grk_amd_encode_tiles call has read its device pixels (not for its results). */
int grk_amd_stream_wait_pixels(grk_amd_ctx* ctx, void* hip_stream);
int grk_amd_fetch_table(grk_amd_ctx* ctx, grk_amd_coded_block* table, uint64_t* total_bytes);
/* The rate-control hook (the host reads grk_plugin_pass::distortionDecrease when it makes quality layers,
 * plugin/plugin_bridge.cpp:214-226, tile/TileProcessor.cpp:320-458): for every code-block of the LATEST grk_amd_encode_tiles call,
 * in table order, the distortion decrease of coding its single HT cleanup pass, in the units T1::getwmsedec gives the passes of the
 * reference's own Tier-1 (t1/t1_part1/T1.cpp:394-414): (w_mct * w_band * stepsize)^2 * sum of q^2 over the block, q the quantised
 * integer magnitude that was coded.  (The reference's own HT encoder leaves the field unset, T1HT.cpp:102-127: on its CPU path an
 * HTJ2K job with several layers has no slopes to work with.)  Not for pipelined sequences: reads the planes of the latest call. */
int grk_amd_block_distortion(grk_amd_ctx* ctx, double* distortion, uint64_t capacity);
/* copy coded bytes [0,total) of the arena to host memory */
int grk_amd_fetch_coded(grk_amd_ctx* ctx, uint8_t* dst, uint64_t nbytes);
/* The same without waiting: `dst` must be pinned (grk_amd_host_alloc); the copy is queued on the context's stream and complete after
 * grk_amd_synchronize -- a host that runs Tier-2 over the table (grk_amd_plan_tile_part) while the bytes cross the link. */
int grk_amd_fetch_coded_async(grk_amd_ctx* ctx, uint8_t* dst, uint64_t nbytes);
/* device pointers for zero-copy consumers (RCCL gather of tile parts, tests) */
void* grk_amd_coded_device_ptr(grk_amd_ctx* ctx);
void* grk_amd_plane_device_ptr(grk_amd_ctx* ctx, int which /*0: ingest planes, 1: Mallat planes*/);
/* (after grk_amd_encode_tiles of 8-bit reversible content the Mallat planes hold int16 coefficients -- same strides
 *  and pitches in elements -- unless the environment says GRK_AMD_PLANES16=0; grk_amd_stage_ht_encode16 takes such planes,
 *  every other stage entry point int32 ones) */
/* the block table of the last encode where it was produced, for exchanges that never touch the host:
 * which 0: uint64 offsets[nblocks], 1: uint32 lengths[nblocks], 2: uint64 bytes used in the arena,
 * 3: uint64[24] diagnostics -- per block class, how many blocks outgrew the capped LDS buffers of the HT encoder and
 *    were coded by its fallback launch (0 on natural images; environment GRK_AMD_LDS_CAP=0 gives every block
 *    worst-case buffers instead) */
void* grk_amd_table_device_ptr(grk_amd_ctx* ctx, int which);
int  grk_amd_synchronize(grk_amd_ctx* ctx);
/* The sub-band coefficients of the latest grk_amd_encode_tiles (one tile), component `comp`, as the reference holds them
 * after its DWT: Mallat layout, int32 (float32 bit patterns when irreversible), dst_stride elements per row.  What the
 * plugin hands the host in its self-check mode (GRK_PLUGIN_STATE_DEBUG, grok.h:1719-1739: the host then runs its own
 * Tier-1 over the plugin's coefficients and compares every code-block). */
int  grk_amd_fetch_coefficients(grk_amd_ctx* ctx, uint32_t comp, int32_t* dst, uint32_t dst_stride);

/* ---- stage entry points (parity tests and per-kernel benchmarks call these) ------------------
 * All pointers are DEVICE pointers; planes are int32 (or float32 bit patterns for 9/7) with
 * row stride grk_amd_plane_stride() and plane pitch grk_amd_plane_elems() -- int16 with the same stride and pitch in elements
 * for grk_amd_stage_ht_encode16 / grk_amd_stage_ht_decode16. */
int grk_amd_stage_ingest_mct(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                             const void* d_pixels, void* d_planes);
/* forward DWT of num_planes planes: d_in (ingest planes) -> d_out (Mallat layout); d_in is
 * left untouched (intermediate LL planes live in context-owned ping-pong buffers). */
int grk_amd_stage_dwt_fwd(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_planes,
                          void* d_in, void* d_out);
/* HT cleanup-encode every block of num_tiles tiles from Mallat planes into the context arena. */
int grk_amd_stage_ht_encode(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                            const void* d_mallat);
/* The same from int16 Mallat planes (same stride and pitch in ELEMENTS): the kernel instances grk_amd_encode_tiles launches for
 * 8-bit reversible content -- two quads per lane for the aligned 64 x 64 blocks, int16 loads at the edges, their fallback launch;
 * the context's GRK_AMD_LDS_CAP setting applies as in an encode.  flags: GRK_AMD_STAGE_HT_ROOM = the instance a pipelined encode
 * launches beside the next frame's DWT.  GRK_AMD_ERR_INVALID for parameters an encode would not keep int16 planes for
 * (irreversible, more than 8 bits, no DWT level). */
#define GRK_AMD_STAGE_HT_ROOM 1u
int grk_amd_stage_ht_encode16(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                              const void* d_mallat16, uint32_t flags);

/* The instances of the block coder that take a per-block drop, on planes and drops the caller chose (device pointers).  d_drops:
 * num_tiles * blocks_per_tile bytes, tile-major in table order.  0 .. 254: that many least significant bit-planes of the block are left
 * out -- the magnitudes are coded as mu >> d under the exponent bound Kmax - d, the row's missing_msbs is Kmax - 1 - d, d is clamped to
 * Kmax - 1 --; a block with d > 0 of which nothing is left behind the shift has length 0.  0xFF: the block is not coded: length 0,
 * missing_msbs Kmax - 1.  d = 0 codes the block as grk_amd_stage_ht_encode does.  planes16 != 0: int16 planes (the conditions of
 * grk_amd_stage_ht_encode16).  The context's GRK_AMD_LDS_CAP setting applies.  d_drops is read in the order of the context's stream
 * (the context keeps a copy of its own for the table's missing_msbs).  A codestream of such rows needs GRK_AMD_CS_BLOCK_MSBS. */
int grk_amd_stage_ht_encode_drops(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                                  const void* d_mallat, int planes16, const uint8_t* d_drops);

/* Tier-2 on the device (the kernels behind grk_amd_assemble_device) over a table of the caller's choosing.  HOST pointers: `table` holds
 * num_tiles x (code-blocks of a tile) rows in the order of grk_amd_fetch_table, whose offsets point into the coded_bytes bytes at
 * `coded`; rows may share bytes; missing_msbs is ignored (GRK_AMD_CS_BLOCK_MSBS: GRK_AMD_ERR_UNSUPPORTED).  flags: GRK_AMD_CS_*.
 * The geometry, the plan and its cache are grk_amd_assemble_device's.  Everything is checked on the host before anything is launched:
 * GRK_AMD_ERR_INVALID for a tile index above 65 535 or a row whose offset + length lies beyond coded_bytes, GRK_AMD_ERR_UNSUPPORTED for
 * a length above grk_amd_t2_max_block_bytes().  Synchronous.  Returns the bytes assembled -- the tile-parts one behind the other from
 * offset 0, read with grk_amd_fetch_assembled -- and their lengths in part_bytes[num_tiles] (optional).  The latest
 * grk_amd_encode_tiles call can still be assembled afterwards. */
int64_t grk_amd_stage_assemble(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                               uint32_t flags, const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes,
                               uint32_t* part_bytes);
/* grk_amd_stage_assemble with every tile divided into tile-parts (GRK_AMD_CS_TP, below): at the caller's packets -- starts[nparts] as
 * grk_amd_write_tile_parts takes them, the same for every tile -- or with starts == NULL / nparts == 0 under the division of `flags`.
 * All checks run on the host before any launch (GRK_AMD_ERR_INVALID for starts that decrease, do not begin at 0, exceed the tile's
 * packets or number more than 255).  The tiles' parts lie one behind the other from offset 0; part_bytes[num_tiles][parts] (optional)
 * are the parts' lengths, grk_amd_assembled_parts() their number per tile.  The bytes are grk_amd_write_tile_parts'. */
int64_t grk_amd_stage_assemble_parts(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                                     uint32_t flags, const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes,
                                     const uint32_t* starts, uint32_t nparts, uint32_t* part_bytes);
/* the longest code-block the device writer takes, in bytes; a longer one makes grk_amd_assemble_device and the whole-image encoders'
 * device route return GRK_AMD_ERR_UNSUPPORTED (the image encoders then take the host writer) */
uint32_t grk_amd_t2_max_block_bytes(void);
/* grk_amd_stage_assemble with the rows' missing_msbs WRITTEN: the zero-bit-plane tag trees in their general form, every block with
 * its own value (the rows of a rate- or quality-targeted encode) -- the tile-parts grk_amd_write_tile_part writes under
 * GRK_AMD_CS_BLOCK_MSBS, which is accepted in `flags` and implied.  The same checks on the host before anything is launched, and
 * GRK_AMD_ERR_UNSUPPORTED for a row whose missing_msbs lies above grk_amd_t2_max_block_msbs() (63: above any Kmax - 1 of this library's
 * geometry).  A zero-length row is included like any other, with whatever missing_msbs it carries. */
int64_t grk_amd_stage_assemble_msbs(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                                    uint32_t flags, const grk_amd_coded_block* table, const uint8_t* coded, uint64_t coded_bytes,
                                    uint32_t* part_bytes);
uint32_t grk_amd_t2_max_block_msbs(void);

/* The statistics kernel of the rate-targeted encodes (KR1, see grk_amd_encode_tiles_rate below) on planes of the caller's choosing.
 * d_mallat: DEVICE planes of num_tiles tiles, int32 (float32 bit patterns for 9/7), or with planes16 != 0 int16 under the conditions of
 * grk_amd_stage_ht_encode16.  The kernel runs over the context's block descriptors for *p, as a rate-targeted call runs it, and E
 * (HOST, uint64 [max_drop + 2][n], row max_drop + 1: SKIP) receives what it wrote.  first_rows == NULL: n is ignored and taken as
 * num_tiles * (code-blocks of a tile), block i of the call is column i.  first_rows (HOST, [num_tiles]) != NULL: the map of a joint
 * table -- block j of tile t is column first_rows[t] + j of rows of n entries; the caller's contents of E are uploaded first, so that
 * every entry the kernel did not write comes back as it went in.  Everything is checked on the host before anything is launched:
 * GRK_AMD_ERR_INVALID for max_drop 0 or above 12, for a first row whose tile would end beyond n, for int16 planes where no encode
 * keeps them (9/7 among them).  Synchronous.  The tables of the latest rate-targeted call stay as they are. */
int grk_amd_stage_rate_stats(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const void* d_mallat, int planes16,
                             uint32_t max_drop, const uint64_t* first_rows, uint64_t n, uint64_t* E);

/* The allocator of the rate-targeted encodes (KR2) on tables of the caller's choosing.  HOST pointers: L uint32 [rows][n] (every entry
 * below 2^31), E uint64 [rows][n], W double [n] (positive), rows = max_drop + 2 whether or not SKIP may be chosen (allow_skip == 0: the
 * last row is not read).  One launch of the kernel for `budget` bytes; drops[n] receives the drop bytes (0 .. max_drop, 0xFF: SKIP)
 * and *result everything the kernel reports: the bytes of the final choice, of the Lagrange solution before the fill and of the
 * shortest choice there is, the final choice's sum of W E, the multiplier, whether the budget is feasible (least_bytes <= budget) and
 * the evaluations the multiplier search made.  A budget below least_bytes is no error of this call: feasible = 0 and the drops are
 * those of the shortest choice.  GRK_AMD_ERR_INVALID, before anything is launched: max_drop 0 or above 12, n 0, a null pointer, an
 * entry of L of 2^31 or more.  Synchronous.  The tables go to buffers of their own: the tables, the budget and the drops of the
 * latest rate-targeted call (grk_amd_rate_tables, grk_amd_rate_last_budget) stay valid. */
typedef struct grk_amd_rate_alloc_result {
    uint64_t block_bytes;    /* the final choice's bytes */
    uint64_t lagrange_bytes; /* ... the Lagrange solution's, before the fill (the shortest choice's where no multiplier was used) */
    uint64_t least_bytes;    /* the fewest bytes any choice takes */
    double   distortion;     /* sum of W_b E over the final choice */
    double   lambda;         /* the multiplier; 0: the finest candidates fit, or the budget is not feasible */
    uint32_t feasible;       /* least_bytes <= budget */
    uint32_t steps;          /* evaluations of the multiplier search: bracketing (at most 200) + 40 bisections; 0: no search */
} grk_amd_rate_alloc_result;
int grk_amd_stage_rate_alloc(grk_amd_ctx* ctx, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop,
                             int allow_skip, uint64_t budget, uint8_t* drops, grk_amd_rate_alloc_result* result);

/* ---- decode: the inverse hot path --------------------------------
 * TileProcessor::decompress T1 + post-T1 for HT blocks: T1HT::decompress (t1/t1_ht/T1HT.cpp:129-179,
 * ojph_decode_codeblock t1/t1_ht/coding/ojph_block_decoder.cpp:989), dequantisation
 * (filters/PostDecompressFilters.h:94-140), inverse DWT (transform/WaveletReverse.cpp:852-936,
 * :1360-1439), inverse MCT + DC shift + clamp (point_transform/mct.cpp:109-465).
 * `table` (host) has one row per code-block in the encoder's enumeration order with the block's
 * byte range inside `coded` and its missing_msbs -- exactly what the host's Tier-2 parser knows
 * after decompress_synch_plugin_with_host (plugin/plugin_bridge.cpp:63-76); length 0 = no data.
 * `pixels` receives the tiles back to back, component-major planar, tight (or as grk_amd_set_decode_pixel_layout says), ceil(prec/8) bytes per
 * sample.  With pixels_on_device != 0 the call is asynchronous: query grk_amd_decode_status().
 * Returns GRK_AMD_ERR_INVALID for a block the reference decoder would reject. */
int grk_amd_decode_tiles(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                         const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes,
                         int coded_on_device, void* pixels, int pixels_on_device);
int grk_amd_decode_status(grk_amd_ctx* ctx);
/* A SEQUENCE of frames: with frames_in_flight = n in 2..8, consecutive grk_amd_decode_tiles calls whose coded bytes and pixels
 * are device buffers are decoded on n internal buffer / stream sets in turn, each queued behind what the caller has on the
 * context's stream at the time of the call, so that frame f + 1's block decoding (serial chains that leave most of the GPU
 * idle) runs beside frame f's dequantisation and inverse transform.  The reference decodes a frame's tiles as pooled tasks
 * (codestream/CodeStreamDecompress.cpp:450-519); this is the same idea across frames.  A call returns when its kernels are
 * queued; a frame's pixels are complete after grk_amd_synchronize (all frames) -- grk_amd_decode_status reports the worst
 * status of all of them.  0 or 1: off (every call on the context's own stream, as before).  Calls with host buffers and
 * grk_amd_decode_region always run on the context itself.
 * Streams and hardware queues: the HIP runtime puts a process's streams on (by default) 4 hardware queues per priority level
 * and kernels that share a queue run in turn; the internal sets therefore use two streams each, and for Part-1 frames (two
 * long kernels per frame) streams of both priority levels in turn (8192x8192x3 12-bit: 15.0 ms one frame at a time, 9.1 with
 * two in flight, 7.2 with six).  A host that decodes such sequences gains a little more from eight hardware queues
 * (GPU_MAX_HW_QUEUES in its environment before its first HIP call) (6.2-6.8 with six); the library leaves the variable alone: it is process-wide, and the
 * encode pipeline beside an RCCL exchange measured 25 % slower on anything but the default. */
int grk_amd_set_decode_pipelining(grk_amd_ctx* ctx, int frames_in_flight);
/* Buffer lifetime in a decode sequence.  With n frames in flight a call's device buffers -- the coded bytes it reads, the pixels
 * it writes -- are in use until THAT frame has been decoded, which is up to n calls later and on streams of the library's own:
 * work the caller queues on the context's stream (or any other) is NOT ordered behind it.  A caller therefore rotates n coded /
 * pixel buffers (as many as frames in flight) and, before it overwrites or reads the buffers it handed over n calls ago -- the
 * ones the NEXT grk_amd_decode_tiles call will reuse the same internal set for --, makes its stream wait:
 *     grk_amd_decode_stream_wait_slot(ctx, stream);   upload frame f's coded bytes on `stream`;   grk_amd_decode_tiles(...);
 * (no host synchronisation: a stream-side wait for the event behind that set's last frame; without a sequence it is
 * grk_amd_stream_wait_results).  grk_amd_synchronize(ctx) remains the blunt form: all frames of all sets. */
int grk_amd_decode_stream_wait_slot(grk_amd_ctx* ctx, void* hip_stream);
/* 8-bit reversible HT tiles are decoded with int16 planes between the block decoder and the inverse DWT (default on; half
 * the bytes of the two HBM-bound halves of the decode), and the inverse 5/3 runs on packed pairs of them, which takes every
 * coefficient and every synthesised LL sample within +-2047 (an 8-bit image's are: |HH| <= 1020 at the top resolution, the
 * LL of every level is image-sized); a stream whose values are not is never decoded to other pixels: a synchronous call (host
 * pixels) decodes it again with int32 planes by itself, an asynchronous one reports GRK_AMD_ERR_RANGE from
 * grk_amd_decode_status() and the caller repeats the call after grk_amd_set_decode_planes16(ctx, 0). */
int grk_amd_set_decode_planes16(grk_amd_ctx* ctx, int on);
/* Bytes per coefficient of the LL / Mallat planes that grk_amd_encode_tiles (decode = 0, device pixels) or grk_amd_decode_tiles
 * (decode = 1) keeps for tiles of these parameters: 2 for 8-bit reversible content (int16 planes: every coefficient provably
 * fits, results identical to the int32 path), else 4.  *packed_levels (may be NULL) = the forward DWT levels that run on packed
 * int16 pairs.  What a roofline figure has to count the plane traffic with (bench.py). */
int grk_amd_plane_sample_bytes(grk_amd_ctx* ctx, const grk_amd_tile_params* p, int decode, uint32_t* packed_levels);
/* Region (windowed) decode of ONE tile -- what grk_decompress_set_window() + grk_decompress() do on the host
 * (grok.h; partial synthesis: transform/WaveletReverse.cpp:1466-2213, tile/SparseBuffer.h): the pixels of the window
 * [x0, x1) x [y0, y1) of the tile, component-major planar, tight (or as grk_amd_set_decode_pixel_layout says, pitches the window's), (x1 - x0) * (y1 - y0) samples per component --
 * bit-identical to the same crop of grk_amd_decode_tiles' output.  Only the code-blocks a sample of the window depends
 * on are entropy-decoded and only the strips / row segments of each DWT level that lead to it are synthesised, so
 * the cost follows the window, not the image.  table / coded describe the whole tile, as for grk_amd_decode_tiles.
 * Needs at least one DWT level and <= 16-bit pixels (GRK_AMD_ERR_UNSUPPORTED otherwise). */
int grk_amd_decode_region(grk_amd_ctx* ctx, const grk_amd_tile_params* p,
                          const grk_amd_coded_block* table, const void* coded, uint64_t coded_bytes, int coded_on_device,
                          uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, void* pixels, int pixels_on_device);
/* Decode at reduced resolution -- grk_decompress -r N, grk_dparameters::cp_reduce (grok.h:692-732; the reference skips the
 * code-blocks of the `reduce` finest resolutions and runs `reduce` fewer inverse DWT levels, TileComponent.cpp:69-170 with
 * numResolutionsToDecompress): the following grk_amd_decode_tiles / grk_amd_decode_region calls return the tile at 1 / 2^reduce
 * of its size, bit-identical to the component the reference returns with cp_reduce = reduce -- for a tile whose origin is off
 * the 2^reduce grid, to its first w x h samples (see grk_amd_reduced_tile_rect).  0 (the default) = full resolution.
 * A call whose tile has fewer DWT levels than `reduce` returns GRK_AMD_ERR_INVALID (the reference refuses cp_reduce >=
 * numresolutions, CodeStreamDecompress.cpp:1604); reduce = num_levels is legal: the LL band, no inverse level.
 *   - p, table and coded are those of the FULL tile, as for a full decode: one row per block of the full tile.  Rows of the
 *     resolutions above num_levels - reduce are ignored and never read (their offsets and lengths need not be valid).
 *   - The segment list of grk_amd_set_decode_segments is still indexed over the full tile's blocks, the lists of
 *     grk_amd_set_decode_qcd / grk_amd_set_decode_steps over the full tile's bands.
 *   - pixels: the reduced tiles back to back, component-major, tight, ceil(prec / 8) bytes per sample -- each
 *     grk_amd_reduced_tile_rect(p, reduce) in size.  grk_amd_decode_region takes its window in the reduced tile's coordinates,
 *     [0, w) x [0, h), and needs at least one remaining DWT level (GRK_AMD_ERR_UNSUPPORTED for reduce = num_levels).
 *   - A decode sequence (grk_amd_set_decode_pipelining) hands the value to its frames like the settings above; it may change from
 *     one frame to the next.
 *   - The grk_amd_stage_* calls and every encode path ignore it: they always work on the full tile.
 *   - A context keeps the device tables of ONE geometry: a call whose reduce differs from the previous call's on the same context
 *     (or internal context of a sequence) rebuilds them behind a host synchronisation of the context's streams.  Interleaving
 *     settings costs that much per change; a host that alternates keeps one context per setting. */
int grk_amd_set_decode_reduce(grk_amd_ctx* ctx, uint32_t reduce);
/* The tile's rectangle at that reduction, on the reduced grid (host only, no context): x0 = ceil(tile_x0 / 2^reduce), x1 =
 * ceil((tile_x0 + tile_w) / 2^reduce), w = x1 - x0, likewise in y -- the reference's rectceildivpow2 of the tile bounds
 * (CodeStreamDecompress.cpp:412-420), i.e. the samples the reference's reduced tile-component holds.  For an origin on the
 * 2^reduce grid that is the component size grk_decompress_read_header reports for a one-tile image with cp_reduce = reduce; for
 * an origin off it the header sizes a component as ceil(width / 2^reduce) (SIZMarker.cpp:54), which can be one column / row
 * more -- samples beyond the tile-component's resolution that the stream does not define.  GRK_AMD_ERR_INVALID for reduce >
 * p->num_levels. */
int grk_amd_reduced_tile_rect(const grk_amd_tile_params* p, uint32_t reduce, uint32_t* x0, uint32_t* y0, uint32_t* w, uint32_t* h);
/* Irreversible streams of another encoder: the SPqcd words (expn << 11 | mant, one per sub-band in QCD
 * order) its QCD marker carries, from which the decode-side step sizes are derived
 * (codestream/Quantizer.cpp:41-63).  count = 0 returns to the exponents this library's encoder writes. */
int grk_amd_set_decode_qcd(grk_amd_ctx* ctx, const uint16_t* words, uint32_t count);
/* The same for a host that already holds the band step sizes: steps[comp * (3 * levels + 1) + band] = the
 * TileBand::stepsize Grok's decoder computed (codestream/Quantizer.cpp:26-66, HT fix-up :54-63 included; note that
 * decompress_synch_plugin_with_host stores HALF of it in the plugin tree, plugin_bridge.cpp:40).  Takes precedence
 * over the QCD words; count = 0 drops it. */
int grk_amd_set_decode_steps(grk_amd_ctx* ctx, const float* steps, uint32_t count);
/* Part-1 blocks with more than one codeword segment (LAZY, TERMALL -- T1::decompress_cblk's segment loop,
 * t1/t1_part1/T1.cpp:1280-1318; Grok's own plugin bridge refuses those, plugin_bridge.cpp:50-61, so this is
 * reachable through this C ABI only).  Segments of block i are first_segment[i] .. first_segment[i+1]-1, their
 * bytes lie end to end at the block's offset.  Applies to the following decode calls; nblocks = 0 returns to
 * one segment per block (length and pass count of the table row).
 * HT blocks (reserved[0] = 0) with the refinement passes of T.814 -- SigProp, MagRef; ojph_decode_codeblock with
 * lengths2 != 0, t1/t1_ht/coding/ojph_block_decoder.cpp:1627-2100, which Grok itself never reaches (T1HT.cpp:158-166) --
 * use the same list: segment 0 = the cleanup pass {Lcup, 1}, segment 1 = {bytes of SigProp + MagRef, 1 or 2 passes}; the
 * table row's length is their sum. */
typedef struct grk_amd_segment { uint32_t length; uint32_t numpasses; } grk_amd_segment;
int grk_amd_set_decode_segments(grk_amd_ctx* ctx, const uint32_t* first_segment, const grk_amd_segment* segments,
                                uint32_t nblocks);
/* HT cleanup decode + dequantisation of every block into Mallat planes (device pointers) */
int grk_amd_stage_ht_decode(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                            const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes,
                            void* d_mallat);
/* The same into int16 Mallat planes (same stride and pitch in ELEMENTS), as grk_amd_decode_tiles keeps them for 8-bit reversible
 * HT tiles, with its range check: a value outside [-bias, bias) -- bias 2048 while the context's inverse transform runs on packed
 * pairs (the default), 32768 with GRK_AMD_DWT_PK=0 -- returns GRK_AMD_ERR_RANGE.  GRK_AMD_ERR_INVALID for irreversible, more
 * than 8 bits, Part-1 blocks, and while a segment list is set (the refinement passes work on int32 planes). */
int grk_amd_stage_ht_decode16(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                              const grk_amd_coded_block* table, const void* d_coded, uint64_t coded_bytes,
                              void* d_mallat16);

/* ---- decode-side stages ------------------------------------------
 * inverse DWT of num_planes Mallat planes -> image-domain planes
 *   (transform/WaveletReverse.cpp:852-936 decompress_tile_53, :1360-1439 decompress_tile_97) */
int grk_amd_stage_dwt_inv(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_planes,
                          const void* d_mallat, void* d_out);
/* inverse RCT/ICT + DC level shift + clamp, planes -> tightly packed pixels (ceil(prec/8) bytes)
 *   (point_transform/mct.cpp:109-177, :186-294, :297-364, :369-465) */
int grk_amd_stage_egress(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles,
                         const void* d_planes, void* d_pixels);

/* average duration (ms) of the named kernel family over the launches since the last reset,
 * measured with HIP events on the context's stream when timing is enabled.
 * which: 0 ingest+mct, 1 dwt (all levels), 2 ht encode kernel (launches on the context's stream), 3 whole
 *        encode_tiles call, 4 ht encode kernel, top resolution (side stream, beside DWT levels >= 1),
 *        5 ht decode, 6 inverse dwt (all levels), 7 egress, 8 ht encode kernel, large-LDS classes (second side stream),
 *        9 the allocator of a rate- or quality-targeted encode (whose trial and final block-coder launches count under 2).
 * One encode runs the ht encode kernel up to three times (2, 4, 8): its time per step is their sum.
 * Pipelined encodes of small frames (a frame's whole chain on one of the side streams, GRK_AMD_FRAME_STREAMS): families 1, 2 and 3
 * are then measured on that stream -- the stream that carries the call -- and 4 / 8 stay empty. */
int    grk_amd_enable_timing(grk_amd_ctx* ctx, int on);
/* K3 of the top resolution beside DWT levels >= 1 on side streams (default on; environment GRK_AMD_OVERLAP=0/1
 * sets the default).  Off = every kernel alone on the GPU, one after the other: what per-kernel durations
 * (roofline figures, rocprofv3 summaries) should be measured with, since co-running kernels stretch each other. */
int    grk_amd_set_overlap(grk_amd_ctx* ctx, int on);
/* Pipelining of consecutive grk_amd_encode_tiles calls (a sequence of frames; default off): the per-encode buffers
 * (Mallat planes, coded arena, block table, allocator state) exist twice and the call returns without joining its side
 * streams, so the next call's DWT runs while the blocks of this one are still being coded.  The results of a call stay
 * valid until the second next call.  Every grk_amd_* function that reads them (fetch_table, fetch_coded, synchronize,
 * decode, the stage entry points) joins first; a caller that consumes grk_amd_coded_device_ptr / _table_device_ptr on
 * its own stream must call grk_amd_synchronize before.  Needs the overlap (above) to be on.
 * on = n >= 2 (up to 7): n + 1 buffer sets in rotation -- the results of a call stay valid until the (n + 1)-th next call, for a
 * consumer that works behind the encoder: n = 2 for the tile-part gather of a tile-sharded job one frame behind
 * (grok_amd/dist.py: the receive sizes have to pass through the host, and with two sets that round trip would sit between
 * consecutive frames), n = k + 1 for k gathers in flight at once (each towards another writer, over another xGMI link). */
int    grk_amd_set_pipelining(grk_amd_ctx* ctx, int on);
/* The number of OTHER buffer sets consecutive encodes of tiles with at least one DWT level rotate through right now (0: every
 * encode writes the same arena -- pipelining off, or the overlap switched off). */
int    grk_amd_get_pipelining(grk_amd_ctx* ctx);
/* Makes `hip_stream` (the caller's, e.g. the one its RCCL collectives run on) wait for the results of the latest encode
 * -- the context's stream and, when pipelined, its side streams -- without blocking the context's own stream: the
 * consumer of grk_amd_coded_device_ptr / grk_amd_table_device_ptr in a pipelined sequence. */
int    grk_amd_stream_wait_results(grk_amd_ctx* ctx, void* hip_stream);
double grk_amd_kernel_ms(grk_amd_ctx* ctx, int which, uint32_t* launches);

/* ---- codestream assembly (host) ----------------------------------
 * Writes a complete Part-15 codestream (SOC SIZ CAP COD QCD COM, then per tile SOT SOD + LRCP
 * packets, EOC) for an image of img_w x img_h cut into tiles of p->tile_w x p->tile_h, given the
 * per-tile block tables + coded bytes produced above (tiles in raster order).
 * Byte-identical to the reference's output for the same parameters. Returns length or <0. */
int64_t grk_amd_write_codestream(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h,
                                 const grk_amd_coded_block* table, const uint8_t* coded,
                                 uint8_t* out, uint64_t cap);

/* A tile-part as a PLAN instead of bytes: what the writer writes itself (SOT .. SOD, packet headers, SOP / EPH) in `literal`, and the
 * tile-part as a list of segments in output order -- kind 0: `len` bytes of `literal` from `src`; kind 1: a code-block's bytes, `len`
 * bytes of the coded buffer from `src` (the table row's offset) -- each with its place `dst` in the tile-part.  Tier-2 is O(#blocks) of
 * host work (~1 ms for the 49 152 blocks of an 8K tile); moving the ~100 MB of coded bytes is then the caller's to spread over host
 * threads or to do on the device (grk_amd_assemble_device), once, into the tile-part's final place.  Returns the tile-part's length;
 * with literal / segments NULL only the sizes (*literal_len, *num_segments). */
typedef struct grk_amd_tp_segment { uint64_t dst, src; uint32_t len, kind; } grk_amd_tp_segment;
int64_t grk_amd_plan_tile_part(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags,
                               const grk_amd_coded_block* tile_table, uint8_t* literal, uint64_t literal_cap, uint64_t* literal_len,
                               grk_amd_tp_segment* segments, uint64_t segment_cap, uint64_t* num_segments);

/* Tier-2 on the device (replaces T2Compress::compressPacket t2/T2Compress.cpp:123-333, the tag trees t1/TagTree.cpp:170-218 and the
 * header's bit stuffing t1/BitIO.cpp:46-175 for this encoder's single-layer HT packets; SOT / PLT / SOD as markers/SOTMarker.cpp:41-72,
 * markers/LengthMarkers.cpp:313-374): the finished tile-parts of the LATEST grk_amd_encode_tiles call (num_tiles tiles of *p; no
 * table needs to be fetched for it), tile i numbered tile_index[i], in call order back to back in a device buffer of the context's,
 * starting at dst_offset (0, or the end of what earlier calls assembled: batches of several geometries append).  flags: GRK_AMD_CS_PLT /
 * SOP / EPH / PROG as grk_amd_write_tile_part, whose bytes these are.  part_bytes[i] (optional) = tile-part i's length (what TLM and
 * the caller's placement need).  Returns the bytes assembled by this call, or < 0.  Three kernels (packet headers; the tile-parts' frames
 * and everybody's place; the gather) and one wait for the sizes; the ~100 MB of an 8K frame's code-blocks are moved once, on the device,
 * to where the file has them.
 * Precondition: ONE packet sequence frames the whole call -- that of a tile at *p's origin (tile_x0, tile_y0) in the progression order
 * of `flags`.  Tiles of one geometry (grk_amd_same_tile_geometry) share it for LRCP and RLCP; from RPCL on the sequence also depends on
 * where a tile lies on the reference grid, and only tiles for which grk_amd_same_tile_packets(p, tile, flags) is 1 may share the call:
 * any other tile's packets would be written in *p's order, which nothing here can detect (the call never sees the tiles' own origins).
 * tile_index[i] <= 65 535 (Isot is 16 bits), else GRK_AMD_ERR_INVALID. */
int64_t grk_amd_assemble_device(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                                uint32_t flags, uint64_t dst_offset, uint32_t* part_bytes);
void* grk_amd_assembled_device_ptr(grk_amd_ctx* ctx);
/* grk_amd_assemble_device for the grk_amd_encode_tiles_rate / grk_amd_encode_tiles_quality call before it: the rows' zero bit-planes --
 * made on the device from the drops the blocks were coded with -- are written (the tile-parts of grk_amd_write_tile_part under
 * GRK_AMD_CS_BLOCK_MSBS, which is accepted in `flags` and implied).  GRK_AMD_ERR_INVALID when the latest encode was not such a call. */
int64_t grk_amd_assemble_rate_device(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                                     uint32_t flags, uint64_t dst_offset, uint32_t* part_bytes);
/* The same without the host: queued on `hip_stream`, which is first made to wait for the encode's results (grk_amd_stream_wait_results);
 * nothing is waited for, nothing comes to the host.  The tile-parts (grk_amd_assembled_device_ptr), their places and lengths and the total
 * (grk_amd_assembled_table_ptr -- 0: uint64[tiles] offsets, 1: uint32[tiles] lengths, 2: uint64[2] {bytes assembled, end}) stay where they are
 * for as many further calls as the encoder rotates buffer sets (grk_amd_set_pipelining): what an exchange needs to send FINISHED tile-parts
 * from device memory ("gather of coded tile-parts over xGMI").  Every asynchronous call of a context uses the same stream.
 * The same precondition: every tile of the call is framed with the packet order of a tile at *p's origin (grk_amd_same_tile_packets). */
int grk_amd_assemble_device_async(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const uint32_t* tile_index,
                                  uint32_t flags, void* hip_stream);
void* grk_amd_assembled_table_ptr(grk_amd_ctx* ctx, int which);
/* Under GRK_AMD_CS_TP (which grk_amd_assemble_device, _rate_device and _async honour: the bytes of grk_amd_write_tile_parts) a tile's
 * parts lie one behind the other; tables 0 and 1 and part_bytes[i] then describe the tile's SPAN -- all its parts --, and
 *   table 3: uint32[tiles][grk_amd_assembled_parts(ctx)] the tile-parts' own lengths (what TLM lists)
 * grk_amd_assembled_parts: the tile-parts per tile of the latest assemble call (1: undivided, table 3 is then table 1). */
uint32_t grk_amd_assembled_parts(grk_amd_ctx* ctx);
/* bytes [offset, offset + nbytes) of the assembled tile-parts to host memory (pinned: one DMA; pageable: through pinned chunks on
 * several copy threads); complete on return */
int grk_amd_fetch_assembled(grk_amd_ctx* ctx, uint64_t offset, uint64_t nbytes, uint8_t* dst);
/* the same queued on the context's stream (dst pinned: grk_amd_host_alloc); complete after grk_amd_synchronize */
int grk_amd_fetch_assembled_async(grk_amd_ctx* ctx, uint64_t offset, uint64_t nbytes, uint8_t* dst);

/* ---- images of any tile layout (tiles / images off the origin, ragged edge tiles) ----------------------------------
 * What SIZ says about the image (ISO 15444-1 B.2, B.3; grok.h grk_image x0..y1, grk_cparameters tx0 ty0 t_width t_height):
 * the image area [x0, x1) x [y0, y1) on the canonical grid and the tile grid anchored at (tx0, ty0) <= (x0, y0).  Tile t
 * (raster order) is its grid cell clipped to the image area (tile/TileProcessor.cpp:100-170). */
typedef struct grk_amd_image_layout {
    uint32_t x0, y0, x1, y1;
    uint32_t tx0, ty0, t_width, t_height;
} grk_amd_image_layout;
int64_t grk_amd_layout_num_tiles(const grk_amd_image_layout* im);
/* *out = *base with tile_w / tile_h / tile_x0 / tile_y0 of tile `tile_index` */
int grk_amd_layout_tile(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t tile_index,
                        grk_amd_tile_params* out);
/* 1 when two tiles can share one grk_amd_encode_tiles / grk_amd_decode_tiles batch: same sub-band and code-block partition,
 * same lifting variant at every level (0: they cannot, < 0: error) */
int grk_amd_same_tile_geometry(const grk_amd_tile_params* a, const grk_amd_tile_params* b);
/* 1 when the two tiles can ALSO share one grk_amd_assemble_device(_async) call under the progression order of `flags`
 * (GRK_AMD_CS_PROG): the same number of components, the same geometry and the same sequence of packets (component, resolution,
 * precinct).  That call frames every tile with the packet order of a tile at its p's origin; for PCRL and CPRL (and, as far as the
 * comparison goes, RPCL) the order depends on where the precinct corners of the resolutions coincide once clipped to the tile, which
 * grk_amd_same_tile_geometry does not compare.  For LRCP and RLCP this is grk_amd_same_tile_geometry plus the component count.
 * (0: they cannot, < 0: error).  Host only. */
int grk_amd_same_tile_packets(const grk_amd_tile_params* a, const grk_amd_tile_params* b, uint32_t flags);
/* The codestream of such an image: table = the tiles' rows one tile after the other, tile t having the
 * grk_amd_tile_num_blocks() rows of ITS parameters (grk_amd_layout_tile).  grk_amd_write_codestream(_ex) is this with the
 * layout {origin of p, img_w x img_h, tiles of p->tile_w x p->tile_h}. */
int64_t grk_amd_write_codestream_layout(const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                        const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                        uint8_t* out, uint64_t cap);
int64_t grk_amd_write_main_header_layout(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags,
                                         const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap);
/* Whole image -> codestream: `pixels` (host) is the image area, component-major planar, row-major, tight (or as grk_amd_set_pixel_layout says), ceil(prec/8)
 * bytes per sample.  Tiles are grouped by geometry and every group is coded as one grk_amd_encode_tiles batch (one group
 * for an image at the origin whose tile size is a multiple of 2^levels x the code-block size); returns the length. */
int64_t grk_amd_encode_image(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                             const void* pixels, uint32_t flags, uint8_t* out, uint64_t cap);

/* ---- rate-targeted encodes: at most N bytes ---------------------------------------------------------------------------------
 * HTJ2K codes a block in one cleanup pass and this encoder writes one layer, so bytes are saved per BLOCK: block b is coded with its
 * d_b least significant bit-planes left out (mu >> d_b under Kmax - 1 - d_b zero bit-planes: a decoder that positions the block by
 * the band's Kmax reconstructs the centre of the coarser bin; QCD, step sizes and guard bits are untouched), or not at all (SKIP).
 * WHICH DECODERS DO: for the 9/7 transform Grok and grk_amd_decode_image scale the block decoder's words by the band's step and return
 * the centres.  For the REVERSIBLE transform both shift those words by the BLOCK's own zero bit-planes (Grok: ShiftHTFilter; this
 * library's HT decoder mirrors it), which cancels the position: a 5/3 block with d planes dropped comes back as mu >> d, and
 * `distortion` below is then not what either of them delivers.  Use these calls with the 9/7 transform unless the decoder is known to
 * position reversible blocks by the band; a successful call on a reversible base that dropped anything leaves a note saying so in
 * grk_amd_last_error ("" otherwise).  The candidates of a block are
 * d = 0 .. Dmax and, with allow_skip, SKIP.  On the device, for every block and candidate c: L[c][b], the exact length from a trial
 * launch of the block coder with d = c everywhere (Dmax + 1 extra launches); E[c][b], the exact sum over the block of
 * (2 q - 2 r_c(q))^2 with q the magnitude a plain encode codes and r_c(q) what a decoder reconstructs (q; 0 where q >> c == 0 and
 * for SKIP; else ((q >> c) << c) + 2^(c - 1); c taken as min(c, Kmax - 1), the drop the coder clamps to, so that a row describes
 * the block as coded); W_b = (w_mct * w_band * stepsize)^2 / 4, the weights of grk_amd_block_distortion.
 * The allocator (one kernel, no per-block data on the host) bisects lambda so that c_b = argmin_c W_b E[c][b] + lambda L[c][b] has
 * the largest total within the budget (lagrange_bytes), then walks the blocks once in table order and moves a block to the next finer
 * candidate while that lowers W_b E and fits what is left.  Runs are reproducible: integer sums and fixed-order double sums only.
 *   grk_amd_encode_tiles_rate   one budget (target_bytes: the code-blocks' bytes) over a batch of same-geometry tiles; the rows
 *                               carry missing_msbs = Kmax - 1 - d_b and belong in a codestream with GRK_AMD_CS_BLOCK_MSBS.  Synchronous.
 *   grk_amd_encode_image_rate   a whole image in a file of at most target_bytes, always: through the host writer with
 *                               GRK_AMD_CS_BLOCK_MSBS; the blocks' budget is the target less what the file spends beside its blocks,
 *                               lowered by the overshoot and tried again (at most 4 rounds) when the written file is still too
 *                               long.  A target at or above the plain file's size gives d = 0 everywhere and the bytes of
 *                               grk_amd_encode_image under GRK_AMD_IMAGE_T2=host, whatever the tiling.  Tiles of several geometries,
 *                               grk_amd_rate::joint = 0: each group of tiles gets its share of the budget by sample count, capped at
 *                               its plain bytes (what it cannot use goes to the other groups), and runs the allocator alone on its
 *                               own tables, made again in every round.  joint = 1: the joint tables below.
 *   grk_amd_encode_image_subsampled_rate, grk_amd_encode_surface_rate
 *                               the same for an image with sub-sampled components (pixels as for grk_amd_encode_image_subsampled)
 *                               and for a video surface (resolved, routed and staged exactly as grk_amd_encode_surface does,
 *                               GRK_AMD_SURFACE_DIRECT included): the file, written by grk_amd_write_codestream_subsampled with
 *                               GRK_AMD_CS_BLOCK_MSBS, is at most target_bytes; a target at or above the plain file's size gives the
 *                               bytes of grk_amd_encode_image_subsampled / grk_amd_encode_surface.  Always over joint tables.
 *   JOINT TABLES                one L, E, W over every block of the image, in the order in which the file's writer takes the table:
 *                               tile by tile (sub-sampled: within a tile run by run, within a run component by component).  The
 *                               order depends neither on how the units are grouped into batches nor on whether a surface unit is
 *                               coded in place or staged, and neither do the file's bytes.  Every batch's statistics and trial
 *                               launches write their columns into these tables, once per call; the allocator then runs once per
 *                               round over all of them: ONE multiplier lambda for every block of every component, the fill in
 *                               joint order.  W_b is the weight of the unit's own geometry, and the distortion the sum over every
 *                               component's own samples (the reference's convention): a sub-sampled component's samples carry NO
 *                               factor dx * dy for the area they stand for.
 *   grk_amd_rate_tables         the tables of the latest of those calls (joint: of the whole image; else of its last geometry
 *                               group), to host memory: which 0 L
 *                               uint32 [Dmax + 2][nblocks], 1 E uint64 [Dmax + 2][nblocks] (row Dmax + 1: SKIP), 2 W double
 *                               [nblocks], 3 the chosen drop bytes uint8 [nblocks] (0xFF: SKIP); GRK_AMD_ERR_OVERFLOW: cap_bytes too small
 *   grk_amd_rate_num_blocks     nblocks of those tables (0: there are none)
 *   grk_amd_rate_last_budget    the blocks' budget the allocator last ran with (a whole-image call: the last round's -- the target
 *                               less what the round before spent beside its blocks)
 *   grk_amd_rate_unit_rows      the units the tables are over (joint: the image's units; else the batch's tiles): returns their
 *                               number, first_row[u] (up to cap entries) = unit u's first row
 * GRK_AMD_ERR_OVERFLOW (the reason in grk_amd_last_error): the target is below what SKIP everywhere -- without allow_skip: Dmax
 * everywhere -- takes, or the four rounds ran out with the file still too long (the message says which).  GRK_AMD_ERR_UNSUPPORTED: while pipelining is on.  Not offered: per-component visual
 * weights, the node, the plugin, Tier-2 on the device, pipelined sequences, several layers. */
typedef struct grk_amd_rate {
    uint64_t target_bytes;   /* the blocks' bytes for grk_amd_encode_tiles_rate; the whole file for grk_amd_encode_image_rate */
    uint8_t  max_drop;       /* Dmax, 0 = default 6, at most 12 */
    uint8_t  allow_skip;
    uint8_t  joint;          /* grk_amd_encode_image_rate: 1 = joint tables; the sub-sampled and surface calls are always joint */
    uint8_t  reserved[5];
} grk_amd_rate;
typedef struct grk_amd_rate_result {
    uint64_t block_bytes;    /* the chosen blocks' bytes, final */
    uint64_t lagrange_bytes; /* ... of the Lagrange solution, before the fill */
    uint64_t file_bytes;     /* grk_amd_encode_image_rate: the file's length */
    double   distortion;     /* sum of W_b E over the chosen candidates, final: the bin-centre model's (see above for 5/3) */
    double   lambda;
    uint32_t passes;         /* allocate + encode rounds taken */
    uint32_t reserved;
} grk_amd_rate_result;
int grk_amd_encode_tiles_rate(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const void* pixels,
                              int pixels_on_device, const grk_amd_rate* rate, grk_amd_coded_block* table, uint64_t* total_bytes,
                              grk_amd_rate_result* result);
int64_t grk_amd_encode_image_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                  const void* pixels, uint32_t flags, const grk_amd_rate* rate, uint8_t* out, uint64_t cap,
                                  grk_amd_rate_result* result);
int grk_amd_rate_tables(grk_amd_ctx* ctx, int which, void* dst, uint64_t cap_bytes);
uint64_t grk_amd_rate_num_blocks(grk_amd_ctx* ctx);
uint64_t grk_amd_rate_last_budget(grk_amd_ctx* ctx);
int grk_amd_rate_unit_rows(grk_amd_ctx* ctx, uint64_t* first_row, uint32_t cap);

/* ---- quality-targeted encodes: the fewest bytes for a PSNR ---------------------------------------------------------------------
 * The other half of rate control: the smallest frame that is at least this good (grk_compress -q).  The tables L, E, W, their joint
 * order, the block coder's drop instances, the host writer with GRK_AMD_CS_BLOCK_MSBS and the readers are those of the rate-targeted
 * encodes above; the allocator is KQ, their allocator's dual, and it runs ONCE per call: headers do not enter a distortion budget, so
 * there are no rounds, and the file is written once.
 * THE BUDGET: D = S * peak^2 * 10^(-target_psnr / 10), peak = 2^prec - 1, S the sum over the components of the component's OWN
 * samples in the image area (a sub-sampled component counts its own samples, with no area factor: the convention W and `distortion`
 * follow; grk_amd_encode_tiles_quality: num_tiles * tile_w * tile_h * num_comps).  target_psnr = +infinity: D = 0.  target_psnr == 0:
 * D = target_distortion, in the units of grk_amd_rate_result::distortion.
 * THE ALLOCATOR (one workgroup, fixed-order sums: runs are reproducible), over candidates c = 0 .. Dmax and, with allow_skip, SKIP:
 *   floor = sum over b of W_b * min_c E[c][b]; feasible = floor <= D.  Not feasible: every block goes to its least-E candidate, the
 *   finer of equal ones, with no search and no trim (the tables of an encode have E[0] = 0 everywhere: floor = 0, always feasible).
 *   dist_at(lambda) = sum of W_b * E[choose(b, lambda)][b] with choose(b, lambda) = argmin_c W_b E[c][b] + lambda L[c][b], the finer
 *   candidate on a tie; in exact arithmetic it does not fall as lambda rises.
 *   The shortest choice -- the smallest L per block, the finer of equally short ones --, if its distortion is <= D, is the answer;
 *   lambda is then reported as +infinity and steps as 0.
 *   Otherwise the search mirrors the rate allocator's, with the same limits: from 1, doubling while the doubled multiplier still fits
 *   (dist_at <= D) or halving until one fits, at most 200 steps; then 40 bisections that keep the LOWER end fitting; lambda = lo.
 *   Halving that never fits ends at lo = 0, which fits when feasible.  The Lagrange choice at lambda gives lagrange_bytes.
 *   The trim, the fill's mirror image, in table order: a block moves to the next coarser candidate (c + 1 within the candidates) while
 *   L strictly falls and delta = W_b * (E[c + 1][b] - E[c][b]) is <= left; then left -= delta.  left starts as D - the Lagrange
 *   choice's distortion.  A block that does not fit is passed over and the walk goes on.
 *   `distortion` is summed afresh over the final choice.
 * D = 0 gives d = 0 everywhere, whatever the tiling: the file is byte for byte that of grk_amd_encode_image (_subsampled, _surface,
 * _packed) under GRK_AMD_IMAGE_T2=host.  The encode calls answer it without the allocator (lambda and steps are reported as 0):
 * nothing may be lost.  The allocator alone -- grk_amd_stage_quality_alloc, and every D > 0 -- does take a coarser candidate of EQUAL
 * error in fewer bytes where a table has one (a block of a few samples: in the model a lone odd magnitude survives one dropped plane).
 * WHAT THE MODEL IS: E measures the planes dropped from the magnitudes a plain encode codes, at the bin centres a decoder that
 * positions a block by the band's Kmax returns.  NOT in `distortion`, `budget` or `psnr`: the 9/7 base quantiser's own error; the
 * transform's departure from orthogonality (W_b weighs a band's error by its synthesis gain as if the bands' errors did not
 * interact, and the clamp of the decoded samples to their range is not modelled); for 5/3, what a block-positioning dequantiser
 * returns (mu >> d, see WHICH DECODERS DO above: a successful 5/3 call that dropped anything leaves the same note in
 * grk_amd_last_error).  The PSNR of decoded pixels therefore differs from `psnr`, and not by little: measured on an MI355X
 * (profiles/quality.txt; 9/7, 8-bit synthetic content, Dmax 6 + SKIP) the decoded pixels were 0.8 to 6.5 dB BETTER than targets of 30
 * to 45 dB -- the call is conservative there: it spends more bytes than the decoded PSNR would need -- and 1.3 to 2.3 dB WORSE than
 * a target of 50 dB, where the plain 9/7 file itself decodes at 50.1 dB: a target near or above the plain file's own PSNR cannot be
 * delivered.  Nothing here promises the gap.
 *   grk_amd_encode_tiles_quality               one budget over a batch of same-geometry tiles; rows as grk_amd_encode_tiles_rate's
 *   grk_amd_encode_image_quality               a whole image, always over joint tables, through the host writer with
 *                                              GRK_AMD_CS_BLOCK_MSBS
 *   grk_amd_encode_image_subsampled_quality, grk_amd_encode_surface_quality, grk_amd_encode_packed_quality
 *                                              the same for the inputs of their rate-targeted twins; the packed call's file is the
 *                                              surface call's for the same samples
 *   grk_amd_rate_tables, grk_amd_rate_num_blocks, grk_amd_rate_unit_rows
 *                                              serve the latest call of either kind; grk_amd_rate_last_budget is 0 after a quality
 *                                              call, grk_amd_quality_last_budget the D the quality allocator last ran with (0 after
 *                                              a rate-targeted call)
 * GRK_AMD_ERR_INVALID: a negative or NaN target_psnr, a negative or NaN target_distortion where it is used, max_drop above 12.
 * GRK_AMD_ERR_UNSUPPORTED: while pipelining is on.  Not offered: what the rate-targeted encodes do not offer. */
typedef struct grk_amd_quality {
    double  target_psnr;        /* dB over all samples of all components; > 0: used; +inf: D = 0 */
    double  target_distortion;  /* used when target_psnr == 0: D in the units of grk_amd_rate_result::distortion, >= 0 */
    uint8_t max_drop, allow_skip, reserved[6];    /* max_drop: Dmax, 0 = default 6, at most 12 */
} grk_amd_quality;
typedef struct grk_amd_quality_result {
    uint64_t block_bytes, lagrange_bytes, file_bytes;     /* the final choice's bytes; the Lagrange choice's, before the trim; the file's (0: tiles) */
    double   distortion, budget, psnr /* model: 10 log10(S peak^2 / distortion), +inf for 0 */, lambda;
    uint32_t steps, reserved;
} grk_amd_quality_result;
int grk_amd_encode_tiles_quality(grk_amd_ctx* ctx, const grk_amd_tile_params* p, uint32_t num_tiles, const void* pixels,
                                 int pixels_on_device, const grk_amd_quality* quality, grk_amd_coded_block* table, uint64_t* total_bytes,
                                 grk_amd_quality_result* result);
int64_t grk_amd_encode_image_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                     const void* pixels, uint32_t flags, const grk_amd_quality* quality, uint8_t* out, uint64_t cap,
                                     grk_amd_quality_result* result);
double grk_amd_quality_last_budget(grk_amd_ctx* ctx);
/* KQ on tables of the caller's choosing, under grk_amd_stage_rate_alloc's rules: HOST pointers, rows = max_drop + 2, everything checked
 * before a launch (GRK_AMD_ERR_INVALID: max_drop 0 or above 12, n 0, a null pointer, an entry of L of 2^31 or more, a D that is
 * negative or NaN), buffers of its own, synchronous; the tables of the latest rate- or quality-targeted call stay valid.  A D below
 * `floor` is no error: feasible = 0 and the drops are those of the least-E choice. */
typedef struct grk_amd_quality_alloc_result {
    uint64_t block_bytes;    /* the final choice's bytes */
    uint64_t lagrange_bytes; /* ... the Lagrange choice's, before the trim (the shortest or the least-E choice's where no multiplier was used) */
    uint64_t shortest_bytes; /* the fewest bytes any choice takes */
    double   distortion;     /* sum of W_b E over the final choice, summed afresh */
    double   floor;          /* sum of W_b min_c E: the least distortion any choice has */
    double   lambda;         /* the multiplier; +infinity: the shortest choice fits; 0: only the least-E choice fits, or not feasible */
    uint32_t feasible;       /* floor <= D */
    uint32_t steps;          /* evaluations of the multiplier search: bracketing (at most 200) + 40 bisections; 0: no search */
} grk_amd_quality_alloc_result;
int grk_amd_stage_quality_alloc(grk_amd_ctx* ctx, const uint32_t* L, const uint64_t* E, const double* W, uint64_t n, uint32_t max_drop,
                                int allow_skip, double D, uint8_t* drops, grk_amd_quality_alloc_result* result);

/* ---- sub-sampled components (4:2:2, 4:2:0 ...; SIZ XRsiz / YRsiz, grok.h grk_image_comp::dx / dy) ------------------------------------
 * Component c of a tile [x0, x1) x [y0, y1) of the reference grid covers [ceil(x0 / dx_c), ceil(x1 / dx_c)) x [ceil(y0 / dy_c),
 * ceil(y1 / dy_c)) of its own samples (tile/TileProcessor.cpp:605-612): grk_amd_layout_tile_comp gives *base with that rectangle.
 * grk_amd_encode_image_subsampled: `pixels` (host) holds the components back to back, component c as ceil(x1 / dx_c) - ceil(x0 / dx_c)
 * columns x ceil(y1 / dy_c) - ceil(y0 / dy_c) rows, tight (the planar layout of a .yuv / raw file).  Runs of consecutive components
 * with equal factors are coded together (the colour transform applies only where components 0..2 are such a run; with
 * other factors base->mct is switched off, as the reference does: CodeStreamCompress.cpp:434-447); the codestream == grk_compress's for the same image (one precinct per resolution or
 * any precinct sizes, the five progression orders, SOP / EPH / TLM / PLT as for any image).  Tier-2 runs on the device under
 * grk_amd_encode_image's rule -- GRK_AMD_IMAGE_T2=host, read per call, selects the host writer; the same file either way (see
 * grk_amd_encode_surface, grk_amd_encode_route_counters).
 * grk_amd_write_codestream_subsampled: the table's rows tile by tile, within a tile component by component, each component with the
 * grk_amd_tile_num_blocks() rows of ITS rectangle (num_comps = 1); out == NULL: only the file's length is returned (`coded` is not read). */
int grk_amd_layout_tile_comp(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t dx, uint32_t dy,
                             uint32_t tile_index, grk_amd_tile_params* out);
int64_t grk_amd_write_codestream_subsampled(const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                            const uint8_t* comp_dx, const uint8_t* comp_dy,
                                            const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                            uint8_t* out, uint64_t cap);
int64_t grk_amd_encode_image_subsampled(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                        const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                        uint8_t* out, uint64_t cap);
/* ... in a file of at most rate->target_bytes (rate-targeted encodes, above) */
int64_t grk_amd_encode_image_subsampled_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                             const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                             const grk_amd_rate* rate, uint8_t* out, uint64_t cap, grk_amd_rate_result* result);
/* ... in the fewest bytes the quality allocator finds for quality->target_psnr (quality-targeted encodes, above) */
int64_t grk_amd_encode_image_subsampled_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                                const uint8_t* comp_dx, const uint8_t* comp_dy, const void* pixels, uint32_t flags,
                                                const grk_amd_quality* quality, uint8_t* out, uint64_t cap, grk_amd_quality_result* result);

/* The same with the optional pointer marker segments of the reference's encoder (grk_compress -L / -X, grok.h
 * grk_cparameters::writePLT / writeTLM; codestream/markers/LengthMarkers.cpp): TLM in the main header (one-byte tile index +
 * four-byte tile-part length, <= 255 tiles), PLT (packet lengths) in every tile-part header. */
#define GRK_AMD_CS_TLM 1u
#define GRK_AMD_CS_PLT 2u
/* SOP marker segments in front of the packets / EPH markers after the packet headers (grk_cparameters::csty bits 0x02 / 0x04,
 * grk_compress -S / -E; t2/T2Compress.cpp:149-164, :321-327) */
#define GRK_AMD_CS_SOP 4u
#define GRK_AMD_CS_EPH 8u
/* progression order (grk_cparameters::prog_order, GRK_PROG_ORDER: 0 LRCP, 1 RLCP, 2 RPCL, 3 PCRL, 4 CPRL) << 8 */
/* The zero-bit-plane tag trees coded from the rows' own missing_msbs (T.800 B.10.2 in its general form) instead of the constant
 * Kmax - 1 every block of a plain encode has: what a table from grk_amd_encode_tiles_rate / grk_amd_stage_ht_encode_drops needs.
 * Without the flag every byte is as before; with it and every row at Kmax - 1 as well.  Taken by the host writers
 * (grk_amd_write_codestream_ex / _layout / _subsampled, grk_amd_write_tile_part; grk_amd_write_main_header accepts it, the header does not
 * change); grk_amd_plan_tile_part and grk_amd_assemble_device(_async) return GRK_AMD_ERR_UNSUPPORTED. */
#define GRK_AMD_CS_BLOCK_MSBS 16u
#define GRK_AMD_CS_PROG_SHIFT 8
#define GRK_AMD_CS_PROG(order) ((uint32_t)(order) << GRK_AMD_CS_PROG_SHIFT)
int64_t grk_amd_write_codestream_ex(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h,
                                    const grk_amd_coded_block* table, const uint8_t* coded, uint32_t flags,
                                    uint8_t* out, uint64_t cap);
/* The pieces of the above, for a tile-sharded job whose ranks write their own tile-parts (parallel writer: every rank sizes
 * its tile-parts, the sizes are exchanged, each rank then knows its offsets in the file -- CodeStreamCompress.cpp:535-603
 * writes the tile-parts in index order).  out == NULL: only the size is returned.
 *   grk_amd_write_main_header  SOC SIZ CAP COD QCD [TLM with tile_part_bytes[tile], needed when flags has GRK_AMD_CS_TLM] COM
 *   grk_amd_write_tile_part    SOT [PLT] SOD + LRCP packets of tile `tile_index`; tile_table = that tile's rows
 *   (the codestream ends with EOC, 0xFFD9) */
int64_t grk_amd_write_main_header(const grk_amd_tile_params* p, uint32_t img_w, uint32_t img_h, uint32_t flags,
                                  const uint32_t* tile_part_bytes, uint8_t* out, uint64_t cap);
int64_t grk_amd_write_tile_part(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags,
                                const grk_amd_coded_block* tile_table, const uint8_t* coded, uint8_t* out, uint64_t cap);
/* ---- tiles divided into tile-parts (grk_compress -u R|L|C; T.800 A.4.2) ----------------------------------------------------
 * Bits 12-13 of `flags`: the division letter.  0: one tile-part per tile, every byte as before.  The rule is the reference's
 * (CodeStreamCompress::get_num_tp, pi_enable_tile_part_generation) for this encoder's one layer: with `pos` the place of the letter in
 * the progression order's name (LRCP, RLCP, RPCL, PCRL, CPRL), a packet's key is its coordinates for the letters 0 .. pos, and a new
 * tile-part starts wherever the key changes.  A tile has as many parts as there are keys -- the product of the letters' extents
 * (R: num_levels + 1, C: num_comps, L: 1) --, whether or not a key has packets: a part without packets is 14 bytes.
 *              R        L                             C
 *   LRCP       R parts  1 (the undivided file)        R x C
 *   RLCP       R        R                             R x C
 *   RPCL       R        refused                       refused
 *   PCRL       refused  refused                       refused
 *   CPRL       refused  refused                       C
 * Refused: GRK_AMD_ERR_UNSUPPORTED -- a P at or before the division letter; more than 255 parts per tile; with GRK_AMD_CS_TLM more than
 * 13 106 parts in the file (one TLM marker segment).  The reason: grk_amd_writer_last_error for the host-only calls,
 * grk_amd_last_error for a context's.
 * A divided tile: its parts one behind the other, the tiles in their order; every part SOT (TPsot = k, TNsot = the tile's parts,
 * Psot = the part's length), with GRK_AMD_CS_PLT the PLT marker segments of its OWN packets (Zplt from 0; none in a part without
 * packets), SOD, its packets unchanged -- SOP's Nsop keeps counting through the tile.  (The reference writes one PLT for the whole tile
 * into the first part; this writer does not copy that.)  With GRK_AMD_CS_TLM the single TLM marker segment lists every tile-part in
 * file order and is the LAST segment of a divided file's main header.
 * Taken by grk_amd_write_codestream_ex / _layout / _subsampled, grk_amd_write_tile_parts, grk_amd_assemble_device(_async),
 * grk_amd_assemble_rate_device and the plain whole-image encoders; GRK_AMD_ERR_UNSUPPORTED from the rate- and quality-targeted calls,
 * grk_amd_plan_tile_part, grk_amd_node_* and the plugin. */
#define GRK_AMD_CS_TP_SHIFT 12
#define GRK_AMD_CS_TP(d)    ((uint32_t)(d) << GRK_AMD_CS_TP_SHIFT)
#define GRK_AMD_TP_R 1
#define GRK_AMD_TP_L 2
#define GRK_AMD_TP_C 3
/* the first packet number of every tile-part of a tile under flags' order and division (non-decreasing; equal neighbours: a
 * tile-part without packets); returns the number of tile-parts, *num_packets the tile's packets; comp_dx / comp_dy NULL: 1.
 * `tile` is the tile on the reference grid (grk_amd_layout_tile).  starts == NULL: the count alone. */
int64_t grk_amd_tile_part_starts(const grk_amd_tile_params* tile, const uint8_t* comp_dx, const uint8_t* comp_dy, uint32_t flags,
                                 uint32_t* starts, uint32_t cap, uint32_t* num_packets);
/* starts / nparts: the division as grk_amd_tile_part_starts gives it, or NULL / 0: taken from flags.  Explicit starts may be any
 * non-decreasing packet numbers <= the tile's packets, starts[0] == 0, 1 <= nparts <= 255 (GRK_AMD_ERR_INVALID otherwise).
 * part_bytes[nparts] (optional): the parts' lengths.  out == NULL: sizes only. */
int64_t grk_amd_write_tile_parts(const grk_amd_tile_params* p, uint32_t tile_index, uint32_t flags, const grk_amd_coded_block* tile_table,
                                 const uint8_t* coded, const uint32_t* starts, uint32_t nparts, uint8_t* out, uint64_t cap, uint32_t* part_bytes);
/* main header whose TLM lists tile-parts: parts_per_tile[tiles], part_bytes in file order */
int64_t grk_amd_write_main_header_parts(const grk_amd_image_layout* im, const grk_amd_tile_params* base, uint32_t flags,
                                        const uint32_t* parts_per_tile, const uint32_t* part_bytes, uint8_t* out, uint64_t cap);
/* why the calling thread's latest host writer call (the three above, grk_amd_write_codestream_*) refused a division */
const char* grk_amd_writer_last_error(void);
/* Random access (the reader's side of markers/LengthMarkers.cpp:91-164): offset, length and tile index of every tile-part
 * of a codestream -- from its TLM marker segments when present (*used_tlm = 1: no byte of a tile-part is read), else by
 * hopping over Psot.  Returns the number of tile-parts (entries beyond `cap` are counted, not stored) or < 0. */
int64_t grk_amd_locate_tile_parts(const uint8_t* cs, uint64_t len, uint64_t* offsets, uint32_t* lengths,
                                  uint16_t* tile_index, uint64_t cap, int* used_tlm);

/* ---- reading a codestream (host only; t2_reader.cpp) and decoding a whole image (decode_image.hip) ----------------------
 * The reader's side of the writers above (CodeStreamDecompress main header + T2Decompress::decompressPacket, t2/T2Decompress.cpp;
 * written from ITU-T T.800 Annex A / Annex B and T.814): what SIZ, COD and QCD say, then every packet header of every tile,
 * which yields the block table grk_amd_decode_tiles takes.  It reads what this library's writers and grk_compress produce:
 *   main header   SOC SIZ CAP COD QCD (Sqcd styles 0 and 2) COM TLM CRG
 *   tile-parts    one per tile, in any tile order; PLT and COM in the tile-part header.  grk_amd_read_packets_parts (below) and the
 *                 decode calls that read a file by themselves also take tiles divided into 1..255 tile-parts
 *   packets       the five progression orders, any precinct sizes, 1..N layers, SOP / EPH, empty packets, blocks that are not
 *                 included, tag trees in their general form, Part-1 codeword segments (TERMALL, LAZY) carried on across
 *                 layers, HT blocks with one pass.  grk_amd_read_packets_refine (below) and the decode calls that read a file by
 *                 themselves also take HT blocks with SigProp and MagRef passes (one HT set: at most 3 passes over all layers)
 *   components    sub-sampled each in its own way (SIZ XRsiz / YRsiz: 4:2:2, 4:2:0, ...): every component of a tile has its own
 *                 rectangle (grk_amd_layout_tile_comp), precinct grid and tag trees, and the position-dependent orders (RPCL,
 *                 PCRL, CPRL) meet its precincts where the factors put them on the reference grid
 * GRK_AMD_ERR_UNSUPPORTED (and the reason in grk_amd_reader_last_error): COC, QCC, RGN, POC, PPM, PPT, PLM, Sqcd style 1, more
 * than one tile-part per tile (grk_amd_read_packets; not _parts, _refine), components of differing precision or sign, more than 4
 * components, more than GRK_AMD_MAX_LEVELS levels, HT blocks with more than one pass (grk_amd_read_packets, _parts) or with more
 * than 3 (_refine: placeholder passes, a second HT set), a custom MCT.  GRK_AMD_ERR_INVALID: anything malformed -- the input is untrusted:
 * no byte outside [cs, cs + len) is read, a packet never runs past its tile-part, a length never wraps. */
typedef struct grk_amd_stream_info {
    grk_amd_image_layout layout;          /* SIZ: image area and tile grid                                                  */
    grk_amd_tile_params  base;            /* SIZ / COD: comps, prec, sgnd, irreversible, mct, levels, code-block exponents, precinct_exp[]
                                             (a resolution with PPx = PPy = 15 reads as 0 = not set); reserved[0] = 1 and reserved[1]
                                             = the style bits for Part-1 blocks; tile_w / tile_h / tile_x0 / tile_y0 = tile 0's   */
    uint32_t flags;                       /* GRK_AMD_CS_TLM / PLT (first tile-part) / SOP / EPH / PROG(order) as found       */
    uint16_t num_layers;
    uint8_t  guard_bits, qstyle;          /* Sqcd >> 5, Sqcd & 31                                                            */
    uint16_t qcd_words[3 * GRK_AMD_MAX_LEVELS + 1];   /* SPqcd: expn << 3 (style 0) or expn << 11 | mant (style 2), as              */
    uint32_t num_qcd;                                 /* grk_amd_tile_layout gives and grk_amd_set_decode_qcd takes them             */
    uint8_t  comp_dx[4], comp_dy[4];      /* XRsiz / YRsiz                                                                   */
    uint32_t num_tiles;
    uint64_t num_blocks;                  /* rows of the whole image: sum over tiles of grk_amd_tile_num_blocks (with a factor
                                             other than 1: over tiles and components, of the component's rectangle as one component) */
} grk_amd_stream_info;
int grk_amd_read_header(const uint8_t* cs, uint64_t len, grk_amd_stream_info* info);
/* Component `comp` of the image in its own samples: *w = ceil(x1 / dx) - ceil(x0 / dx) columns, *h = ceil(y1 / dy) - ceil(y0 / dy)
 * rows (W x H for factors of 1); host only.  What sizes the planes grk_amd_decode_image writes for a sub-sampled stream. */
int grk_amd_stream_comp_size(const grk_amd_stream_info* info, uint32_t comp, uint32_t* w, uint32_t* h);
/* The block table of the whole image.  rows: tile after tile in tile-index order, tile t with the rows of ITS parameters
 * (grk_amd_layout_tile) in grk_amd_tile_layout order: the table grk_amd_write_codestream_layout takes and grk_amd_decode_tiles takes
 * per tile.  A stream with a sub-sampling factor other than 1: within a tile component after component, component c with the rows
 * of its rectangle (grk_amd_layout_tile_comp, num_comps = 1) -- the table grk_amd_write_codestream_subsampled takes; the rows of a
 * run of components with equal factors are the table of one grk_amd_decode_tiles call with num_comps = the run's length.
 * missing_msbs as grk_amd_decode_tiles wants it: HT = zero bit-planes; Part-1 = numbps | numpasses << 8 with numbps =
 * band exponent + guard bits - 1 - zero bit-planes; a block without data has length 0.
 * Where a block's bytes lie in one piece in the file, rows[i].offset is their position in `cs`: nothing is copied, the
 * codestream is the coded buffer.  A block whose bytes come in several pieces (several layers) gets an offset at or behind `len`,
 * in an APPENDIX; `moves` (src in cs, dst in the appendix counted from 0, len; kind 1) say how to fill it.  The coded buffer of a
 * decode is then cs followed by *appendix_bytes bytes.  A single-layer stream has neither.
 * first_segment [num_blocks + 1] / segments: every block's codeword segments as grk_amd_set_decode_segments takes them.
 * `info` is what grk_amd_read_header gave for the same bytes.  threads: host threads to parse on (0 = 1, at most 16): with PLT the
 * precincts of a tile are independent, without it the tiles are.  Every parsed packet is checked against its PLT entry.
 * Returns the number of rows; with rows == NULL only the sizes (*num_segments, *num_moves, *appendix_bytes);
 * GRK_AMD_ERR_OVERFLOW when a capacity is too small. */
int64_t grk_amd_read_packets(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                             grk_amd_coded_block* rows, uint64_t row_cap,
                             uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                             grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
/* grk_amd_read_packets for a codestream whose tiles may be divided into TILE-PARTS (what `grk_compress -u R|L|C`, the cinema and
 * broadcast profiles and any writer that streams a tile resolution by resolution produce), asked for by name; signature and
 * contract are grk_amd_read_packets', which keeps refusing a second tile-part of a tile.  A tile's packet sequence is its
 * tile-parts' bodies end to end, each body a whole number of packets: rows, first_segment, segments, moves and *appendix_bytes are
 * those of the undivided file, every offset and every move's src the byte's place in THIS file; nothing is copied for a
 * single-layer file.  Taken on top of everything grk_amd_read_packets takes:
 *   1..255 tile-parts per tile, at most 65535 in the file; a tile's in TPsot order 0, 1, 2, ... in the file, the tile-parts of
 *   different tiles interleaved in any way; TNsot 0 ("not said here") or the tile's count in any mixture, 0 in every one included;
 *   Psot 0 in the file's last tile-part only; tile-parts that hold no packet; TLM with one entry per tile-part in file order (every
 *   Stlm form grk_amd_locate_tile_parts reads) or none; PLT and COM in every tile-part header, a tile-part's PLT listing its own
 *   packets.  A tile whose every tile-part that holds packets carries PLT for exactly those is parsed precinct by precinct on
 *   `threads` threads; any other tile as one chain in file order, the PLT entries that are present held against the packets read.
 * GRK_AMD_ERR_INVALID, the reason naming tile and tile-part: a TPsot that is missing, repeated or out of file order; two different
 * non-zero TNsot of one tile; a TNsot not above a TPsot seen, or above the tile-parts found; a packet that runs past the end of its
 * tile-part; packets left over or missing at the tile's last tile-part; PLT lengths that do not add up to their tile-part; a Psot
 * that leaves the stream; a tile without a tile-part.  GRK_AMD_ERR_UNSUPPORTED: COD / QCD / COC / QCC / RGN / POC / PPT in a
 * tile-part header, a 256th tile-part of a tile, more than 65535 in the file; HT blocks with more than one pass, as
 * grk_amd_read_packets.  grk_amd_read_header's flags describe the first tile-part. */
int64_t grk_amd_read_packets_parts(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                   grk_amd_coded_block* rows, uint64_t row_cap,
                                   uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                   grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
/* grk_amd_read_packets_parts for an HTJ2K codestream whose code-blocks carry REFINEMENT passes (what an HT encoder writes for a
 * file with quality layers: later layers add SigProp and MagRef to a block's cleanup pass), asked for by name; signature and
 * contract are grk_amd_read_packets_parts' -- tile-parts included --, which keeps refusing an HT block's second pass, as does
 * grk_amd_read_packets.  The signalling is T.814's over T.800 B.10.7: an HT block's passes form one HT set, Cleanup, SigProp,
 * MagRef, numbered across all layers.  The cleanup pass is a codeword segment of its own, SigProp and MagRef share the next one;
 * a segment's length field has Lblock + floor(log2 k) bits for the k passes of that segment in the contribution, and a segment
 * filled by two contributions (SigProp in one layer, MagRef in a later one) accumulates its length.  For an HT block:
 *   rows[i].missing_msbs   the zero bit-planes, as ever
 *   segments               {Lcup, 1} alone, or {Lcup, 1}, {Lref, 1 | 2}: what grk_amd_set_decode_segments takes for the HT block
 *                          decoder (a refinement segment of 0 bytes decodes as the cleanup pass alone)
 *   moves / the appendix   a block whose bytes arrive in more than one layer, exactly as a Part-1 block's
 * GRK_AMD_ERR_UNSUPPORTED, the reason "... an HT code-block with more than one pass of a kind (N passes: placeholder passes or a
 * second HT set)": more than 3 passes in a block's first contribution or over all its layers.  Those are placeholder passes or
 * a second HT set; no encoder or decoder this library was built against writes or reads them, so how their lengths are signalled
 * is not guessed here.  A Part-1 file is read as grk_amd_read_packets_parts reads it. */
int64_t grk_amd_read_packets_refine(const uint8_t* cs, uint64_t len, const grk_amd_stream_info* info, uint32_t threads,
                                    grk_amd_coded_block* rows, uint64_t row_cap,
                                    uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                    grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
/* why the calling thread's latest grk_amd_read_header / grk_amd_read_packets / _parts / _refine refused ("" after a success) */
const char* grk_amd_reader_last_error(void);
/* Codestream -> pixels (Route C, decode; CodeStreamDecompress::decompress, codestream/CodeStreamDecompress.cpp:450-519).
 * cs: the codestream, host memory.  pixels: the image area, component-major planar, tight (or as grk_amd_set_decode_pixel_layout says; cap >= grk_amd_pixel_bytes of the image), ceil(prec / 8) bytes per sample -- the
 * layout grk_amd_encode_image takes; cap: its size in bytes.  pixels_on_device != 0: a device pointer, and the call is asynchronous
 * behind the reader (grk_amd_decode_status joins and reports).
 * The bytes are uploaded once while the host reads the packet headers; blocks of several pieces are gathered on the device; the
 * tiles are grouped by geometry, every group is one grk_amd_decode_tiles batch, and a placement kernel puts a group's tiles at
 * their rectangles (a one-tile image is decoded straight into `pixels`).  The QCD words and segment lists the call sets on the
 * context are put back before it returns.
 * Sub-sampled components (a factor other than 1 in SIZ): the unit of decoding is a tile's run of consecutive components with equal
 * factors; the units are grouped by geometry and batched like tiles.  `pixels` then holds one plane per component, back to back:
 * component c of grk_amd_stream_comp_size columns by rows, tight -- the layout grk_amd_encode_image_subsampled takes; a one-tile image
 * is decoded run by run straight into its planes.  The colour transform applies where components 0..2 form one run.
 * grk_amd_set_decode_upsample(ctx, on != 0) (context state, default off): every component of such a stream is delivered on the
 * reference grid instead, W x H, so that `pixels` is the ordinary image and grk_amd_set_decode_pixel_layout applies to it in full.  No
 * interpolation: the image sample at reference-grid position (gx, gy) is the component's sample (floor(gx / dx), floor(gy / dy)) --
 * each sample repeated over its dx x dy cell -- and 0 where that sample does not exist, i.e. left of dx * ceil(X0 / dx) or above
 * dy * ceil(Y0 / dy): a strip that exists only when the image origin (X0, Y0) is no multiple of the factors (grk_decompress
 * --upsample does the same).  The units are then placed by a kernel that writes every sample's cell, a one-tile image included.  A
 * stream without sub-sampling decodes the same with the switch on and off.
 * GRK_AMD_ERR_UNSUPPORTED: what the reader refuses, a context with grk_amd_set_decode_reduce != 0, an HT stream whose QCD exponents
 * differ from the ones this library derives for a unit's geometry (HT blocks are decoded against those), a COD that asks for the
 * colour transform across components of different size, and a decode pixel layout other than the default for a sub-sampled stream
 * while upsampling is off.  The int16-plane rule (GRK_AMD_ERR_RANGE, grk_amd_set_decode_planes16) holds
 * per group: with host pixels such a group is decoded again with int32 planes by the call itself, with device pixels
 * grk_amd_decode_status reports it. */
int grk_amd_decode_image(grk_amd_ctx* ctx, const uint8_t* cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device);
int grk_amd_set_decode_upsample(grk_amd_ctx* ctx, int on);
/* launches of the gather (which = 0) and placement (which = 1: plain and upsampling) kernels by this context's grk_amd_decode_image calls so far */
uint64_t grk_amd_decode_image_launches(grk_amd_ctx* ctx, int which);
/* A VIEW of the image: at reduced resolution (grk_decompress -r N, grk_dparameters::cp_reduce) and / or a window of it
 * (grk_decompress_set_window) -- proxies and thumbnails of a master, a viewport of a very large image.
 *   reduce r   component k of the image becomes [ceil(ceil(X0 / dx) / 2^r), ceil(ceil(X1 / dx) / 2^r)) x the same in y; tile t delivers
 *              the rectangle grk_amd_reduced_tile_rect gives, and those rectangles partition the image.  Bit-identical to the
 *              reference's reduced image -- with an origin off the 2^r grid, to its top-left w x h samples: the reference sizes
 *              the image from its width (one row / column more that the resolutions do not hold; see grk_amd_reduced_tile_rect).
 *              r > the stream's levels: GRK_AMD_ERR_INVALID; r = levels is legal (the LL band).
 *   window     [x0, x1) x [y0, y1) in samples of the (reduced) image, counted from ITS top-left sample (not the canvas: what
 *              grk_decompress_set_window does); bit-identical to that crop of the whole view.  GRK_AMD_ERR_INVALID: x1 <= x0 or
 *              y1 <= y0 (other than all four 0 = no window), a window outside the view's image.
 * GRK_AMD_ERR_UNSUPPORTED: a window of a stream with sub-sampled components (upsampling on or off), a reduce other than 0 of such a
 * stream while grk_amd_set_decode_upsample is on.  view == NULL or all-zero: exactly grk_amd_decode_image.
 * `pixels` is the view's image -- component k of grk_amd_image_view_size -- and everything grk_amd_decode_image says about it holds
 * with the view's sizes and pitches: host or device pixels, grk_amd_set_decode_pixel_layout, tight planes back to back for
 * sub-sampled components, the int16-plane rule and grk_amd_decode_status, the context's settings put back on return.
 * Only the touched tiles -- those whose rectangle meets the window -- are read, uploaded and decoded: their tile-parts are found
 * through TLM or the Psot chain, the packet reader runs over them alone, and their bytes travel as a compact buffer (a view that
 * touches every tile uploads the codestream as grk_amd_decode_image does).  Under reduce the blocks of the dropped resolutions are
 * neither gathered nor decoded.  A window of a ONE-tile stream is decoded with grk_amd_decode_region, so that the cost follows the
 * window (where that call's conditions hold: a DWT level left, samples of at most 16 bits; else as below).  In a multi-tile
 * stream the touched tiles are decoded whole and the placement kernel clips them to the view: partial tiles of multi-tile streams
 * are decoded whole, the cost follows the touched tiles.
 * The reduce is a parameter of the call, not the context's: like grk_amd_decode_image this call refuses (GRK_AMD_ERR_UNSUPPORTED) a
 * context whose grk_amd_set_decode_reduce is not 0 or that has a decode sequence. */
typedef struct grk_amd_image_view {
    uint32_t reduce;            /* 0 = full size; the N finest resolutions dropped, as grk_decompress -r N */
    uint32_t x0, y0, x1, y1;    /* window [x0, x1) x [y0, y1) in samples of the (reduced) image, relative to its top-left sample;
                                   all four 0 = the whole image */
} grk_amd_image_view;
/* host only: component `comp` of the view: *w x *h samples (the size of its plane in `pixels`) */
int grk_amd_image_view_size(const grk_amd_stream_info* info, const grk_amd_image_view* view, uint32_t comp, uint32_t* w, uint32_t* h);
/* host only, no context: the plan of the call.  tiles [tile_cap]: the touched tiles in index order, *num_tiles of them; units [cap]:
 * per touched tile and run of components of one size (one run without sub-sampling) what its decode delivers -- w x h samples, 0
 * where nothing of the unit is left at this reduce -- and where that rectangle starts in the view's plane of those components:
 * (x, y), signed -- it may start left of / above the view; whole = 1 when the view holds all of it.  Returns the number of units
 * (tiles, units may be NULL: only the counts); GRK_AMD_ERR_OVERFLOW when a capacity is too small, else the refusals above. */
typedef struct grk_amd_view_unit {
    uint32_t tile, first_comp, num_comps;
    uint32_t w, h;
    int32_t  x, y;
    uint32_t whole;
} grk_amd_view_unit;
int64_t grk_amd_plan_image_view(const grk_amd_stream_info* info, const grk_amd_image_view* view, uint32_t* tiles, uint64_t tile_cap,
                                uint64_t* num_tiles, grk_amd_view_unit* units, uint64_t cap);
int grk_amd_decode_image_view(grk_amd_ctx* ctx, const uint8_t* cs, uint64_t len, const grk_amd_image_view* view,
                              void* pixels, uint64_t cap, int pixels_on_device);
/* cumulative per context: which = 0 tiles whose packets a grk_amd_decode_image / grk_amd_decode_image_view call read, 1 codestream
 * bytes those calls uploaded */
uint64_t grk_amd_decode_image_counters(grk_amd_ctx* ctx, int which);

/* ---- a codestream that lies in DEVICE memory, read where it lies ---------------------------------------------------------------
 * Every grk_amd_encode_*_device call leaves its file (SOC .. EOC) in device memory; so do peer and storage DMA.  These calls read
 * such a file without bringing its body to the host: the packet headers are parsed by kernels (KL: the tile-parts located, KH: the
 * tile-part headers with PLT, KC: the packets, one wave per chain -- with PLT a packet, without a tile).  The first three take
 * files of ONE quality layer, HT or Part-1 without LAZY / TERMALL; everything else is GRK_AMD_ERR_UNSUPPORTED before any launch --
 * several layers and LAZY / TERMALL are read by the _ex calls below, which are asked for by name.  d_cs is read in the order of the
 * context's stream; every call here but a decode into device pixels returns synchronised.
 *
 * grk_amd_read_header_device: grk_amd_read_header for such a stream.  Only the main header comes to the host: a first copy of
 *   GRK_AMD_READ_DEVICE_FIRST_COPY bytes and, where the header is longer (a long COM, a TLM of thousands of tiles), a second copy
 *   of the rest.  *info is what grk_amd_read_header gives for the same bytes.
 * grk_amd_read_packets_device: grk_amd_read_packets for such a stream: the rows (HOST memory; NULL: counted only), field for field
 *   what grk_amd_read_packets gives, or the code it gives with threads = 1; grk_amd_last_error names the tile and the packet.
 *   One layer: no segment lists, no moves.  Returns the number of rows.
 * grk_amd_decode_image_device: grk_amd_decode_image for such a stream: the stream is the coded buffer, nothing of its body goes
 *   either way over the link; the rows come to the host once (grk_amd_decode_tiles takes a host table).  Pixels, layouts,
 *   up-sampling, the int16-plane rule and the refusals on the context are grk_amd_decode_image's.
 * grk_amd_read_device_counters: 0 bytes copied device -> host by these calls, 1 bytes copied host -> device by the reader (the
 *   plan's descriptors, once per kind of stream; TLM's places), 2 launches of KC, 3 chains parsed. */
#define GRK_AMD_READ_DEVICE_FIRST_COPY 4096
int grk_amd_read_header_device(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, grk_amd_stream_info* info);
int64_t grk_amd_read_packets_device(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, const grk_amd_stream_info* info,
                                    grk_amd_coded_block* rows, uint64_t row_cap);
int grk_amd_decode_image_device(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device);
uint64_t grk_amd_read_device_counters(grk_amd_ctx* ctx, int which);
/* The GENERAL reader of a stream in device memory, asked for by name (the three calls above keep what they take and refuse): 1 .. N
 * quality layers, HT blocks of one pass in all, Part-1 blocks of every style grk_amd_read_packets takes -- LAZY and TERMALL segments
 * carried on across layers among them --, with or without PLT / TLM / SOP / EPH, every progression order, precinct grid, tile
 * layout and sub-sampling.  It refuses what grk_amd_read_packets refuses, with its code.  KL and KH as above; KC-L: one wave per
 * chain -- with PLT a precinct with its packets of every layer, without a tile in file order -- logs what each contribution adds;
 * KF finishes the rows and scans them (first_segment, the appendix, the moves); KP places the logs' records.
 *
 * grk_amd_read_packets_device_ex: grk_amd_read_packets for such a stream, with that call's contract: rows == NULL returns only the
 *   sizes; GRK_AMD_ERR_OVERFLOW when a capacity is too small (or moves == NULL where there are moves); offsets at or behind `len`
 *   point into an appendix of *appendix_bytes; moves have kind 1, src in the stream and dst counted from 0 in the appendix.  All
 *   output arrays are HOST memory; first_segment has rows + 1 entries.  rows, first_segment, segments and *appendix_bytes are
 *   grk_amd_read_packets' field for field; the moves are its moves as a set, here in the order of their dst.
 * grk_amd_decode_image_device_ex: grk_amd_decode_image_device on top of it.  Without an appendix -- every single-layer file, LAZY /
 *   TERMALL included, and layered files whose blocks all have one piece -- the stream is the coded buffer, nothing is copied.  With
 *   one, the context stages [stream | appendix] in its own coded buffer (one device-to-device copy of `len` bytes: the decoders take
 *   one coded base) and the gather fills the appendix from moves that never leave the device.  d_cs is only read, and nothing is
 *   assumed about memory behind d_cs + len.
 * grk_amd_read_device_counters: 4 bytes the _ex decode copied device to device, 5 launches of KC-L. */
int64_t grk_amd_read_packets_device_ex(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, const grk_amd_stream_info* info,
                                       grk_amd_coded_block* rows, uint64_t row_cap,
                                       uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                       grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
int grk_amd_decode_image_device_ex(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, void* pixels, uint64_t cap, int pixels_on_device);
/* grk_amd_read_packets_device_parts: grk_amd_read_packets_device_ex for a stream whose tiles may be divided into tile-parts, asked for
 * by name: that call's signature and contract, built on the general reader (KC-L, KF, KP: 1 .. N layers, every style).  Field for
 * field what grk_amd_read_packets_parts returns -- the moves as a set --, or the code that call gives with threads = 1.  KL-P (one
 * workgroup) takes every tile-part of the file: TLM's places from the host, or one lane along the Psot chain (at most len / 14 + 1
 * hops); all lanes check the SOTs and count the tile-parts per tile, a scan gives every tile its slice of a part table, a tile-part
 * goes to slice + TPsot.  The status word and the located count (one word) come to the host behind it: KH-P's grid is the file's
 * tile-parts.  KH-P: a workgroup per tile-part walks its header and counts its PLT entries; a workgroup per tile scans the counts,
 * decides whether the tile is a PLT tile, and assembles entries and packet starts.  KC-L then bounds a packet by the end of the
 * tile-part it starts in and steps from body to body where it reads a tile in file order.
 * grk_amd_decode_image_device_ex takes such files without a switch: a file that KL refuses for a second tile-part is read again
 * this way (a file with one tile-part per tile goes exactly the way it went); grk_amd_decode_image_device keeps its refusal.
 * grk_amd_read_device_counters: 6 launches of KL-P / KH-P (three per read). */
int64_t grk_amd_read_packets_device_parts(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, const grk_amd_stream_info* info,
                                          grk_amd_coded_block* rows, uint64_t row_cap,
                                          uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                          grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
/* grk_amd_read_packets_device_refine: grk_amd_read_packets_device_parts for an HTJ2K stream whose code-blocks carry refinement
 * passes, asked for by name: that call's signature and contract.  Field for field what grk_amd_read_packets_refine returns -- the
 * moves as a set --, or the code that call gives with threads = 1.  The same kernels: the plan sizes the logs for two segments,
 * min(layers, 3) pieces and their sum less one segment records per row, and KC-L's parse core fills an HT block's segments 1, 2 by
 * the style word it is handed.  grk_amd_decode_image_device_ex takes such files without a switch: a file that KC-L refuses for
 * an HT block's second pass is read again this way, the segment lists come to the host, and blocks with a second segment are
 * refined by K5c on int32 planes; grk_amd_decode_image_device and the other reader calls keep their refusal. */
int64_t grk_amd_read_packets_device_refine(grk_amd_ctx* ctx, const void* d_cs, uint64_t len, const grk_amd_stream_info* info,
                                           grk_amd_coded_block* rows, uint64_t row_cap,
                                           uint32_t* first_segment, grk_amd_segment* segments, uint64_t seg_cap, uint64_t* num_segments,
                                           grk_amd_tp_segment* moves, uint64_t move_cap, uint64_t* num_moves, uint64_t* appendix_bytes);
/* The placement kernel with clipping (device pointers; queued on the context's stream): as grk_amd_place_tiles_device, but unit i
 * goes to the SIGNED position (pos[2 i], pos[2 i + 1]) of the destination's planes and only what falls inside img_w x img_h is
 * written (a unit wholly outside: nothing).  channels = 0: ncomp planes; channels != 0: the units and the destination hold
 * interleaved pixels of `channels` samples (ncomp is not used), cut by whole pixels. */
int grk_amd_place_tiles_clipped_device(grk_amd_ctx* ctx, const void* tiles, uint32_t ntiles, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                       uint32_t channels, const int32_t* pos, void* image, uint32_t img_w, uint32_t img_h);
/* The two kernels alone (device pointers; queued on the context's stream):
 * gather: moves[i] = `len` bytes from src_base + src to dst_base + dst (moves in host memory, checked against the two sizes);
 * placement: ntiles tiles of w x h samples, ncomp components, bps bytes per sample, back to back at `tiles`, tile i to
 * (rects[2 i], rects[2 i + 1]) = (x, y) of planes of img_w x img_h samples at `image` (rects in host memory). */
int grk_amd_gather_device(grk_amd_ctx* ctx, const grk_amd_tp_segment* moves, uint64_t num_moves, const void* src_base, uint64_t src_bytes,
                          void* dst_base, uint64_t dst_bytes);
int grk_amd_place_tiles_device(grk_amd_ctx* ctx, const void* tiles, uint32_t ntiles, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                               const uint32_t* rects, void* image, uint32_t img_w, uint32_t img_h);
/* upsampling placement: the same units, of a component sub-sampled by (dx, dy); unit i's first sample is sample (origins[2 i],
 * origins[2 i + 1]) of the component.  Sample (x, y) of the component goes to every sample of [x dx, (x + 1) dx) x [y dy, (y + 1) dy)
 * of the reference grid that lies in the image area [img_x0, img_x0 + img_w) x [img_y0, img_y0 + img_h); `image`: ncomp tight planes
 * of that area.  GRK_AMD_ERR_INVALID ("... outside the image") when a sample's cell starts outside the area.  The strip no cell
 * covers (see grk_amd_decode_image) is not written by this call. */
int grk_amd_place_upsampled_device(grk_amd_ctx* ctx, const void* tiles, uint32_t nunits, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                   const uint32_t* origins, uint32_t dx, uint32_t dy, void* image, uint32_t img_x0, uint32_t img_y0,
                                   uint32_t img_w, uint32_t img_h);

/* ---- video surfaces: NV12, I420, NV16, P010 ... (surface_plan.cpp, surface.cpp, kernels_surface.hip) --------------------------------
 * What sub-sampled content is held in on a GPU: a video decoder or encoder, a capture card and hardware frames of a media
 * framework hold a Y plane with a row pitch and then one plane of interleaved Cb / Cr pairs (NV12, NV21, NV16) or two pitched chroma
 * planes (I420, YV12), with 16-bit samples for 10- and 12-bit video.  A SURFACE describes such a buffer component by component:
 * sample (x, y) of component c lies at base + comp[c].offset + y * comp[c].row_pitch + x * comp[c].step * bps, bps = ceil(prec / 8),
 * host endian; sample (0, 0) is the component's first sample of the image area and the component is
 * grk_amd_stream_comp_size columns by rows (the ceil(x / dx) formulas of grk_amd_encode_image_subsampled above).
 * A sample v of component c is stored as v << comp[c].shift: shift = 0 is LSB-aligned (planar I010), shift = 8 * bps - prec is
 * MSB-aligned (the P010 / P012 / P016 family of hardware video: 10 bits << 6).  An encode reads word >> shift -- what lies in the low
 * `shift` bits of the caller's memory is discarded, not checked --, a decode writes v << shift with the low bits zero.  The shift is
 * per component and moves no byte: sizes, placements and the rules below do not depend on it.
 * Rules (GRK_AMD_ERR_INVALID): offset and row_pitch are multiples of bps, a non-zero pitch covers at least one row
 * (((w_c - 1) * step + 1) * bps), step <= 4, prec + shift <= 8 * bps, at most 4 components; prec > 16: GRK_AMD_ERR_UNSUPPORTED.
 * Two components of a DESTINATION (decode) may not share a byte.  Accepted placements of two components: disjoint extents;
 * interleaved partners (equal pitch and step, offsets k * bps apart, 0 < k < step); side by side (equal pitch, the byte ranges of
 * their rows inside a pitch disjoint and not wrapping).  Any other overlap: GRK_AMD_ERR_INVALID.  An encode only reads: any overlap. */
typedef struct grk_amd_surface_comp {
    uint64_t offset;     /* bytes from the surface's base to the component's first sample */
    uint64_t row_pitch;  /* bytes between rows; 0 = tight: ((w_c - 1) * step + 1) * bps */
    uint32_t step;       /* samples from one sample of a row to the next: 1 = a plane of its own, 2 = every other sample (chroma of
                            NV12) ... 4; 0 reads as 1 */
    uint32_t shift;      /* zero bits below the sample in its container: 0 = LSB-aligned, 16 - prec = P010-style */
} grk_amd_surface_comp;
typedef struct grk_amd_surface { grk_amd_surface_comp comp[4]; } grk_amd_surface;
/* host only: bytes from the base to the end of the last sample of any component; 0 for an invalid surface, *why (may be NULL) then
 * points to the reason (a string of the library's). */
uint64_t grk_amd_surface_bytes(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                               const grk_amd_surface* surface, const char** why);
/* host only: the surface and the factors of a named format for the image area of `im` with samples of `prec` bits.  pitch: the luma
 * row pitch in bytes, 0 = the smallest valid one; interleaved chroma rows take `pitch`, planar chroma rows of the 4:2:x forms
 * pitch / 2 rounded up to a multiple of bps, I444's planes `pitch`.  Planes follow each other at rows x pitch.  NV21 / YV12: Cr (V) lies
 * first in memory -- component order stays Y, Cb, Cr.  P016 / P216: the layout of NV12 / NV16 with two bytes per sample and
 * shift = 16 - prec on all three components -- prec 10: P010 / P210, 12: P012 / P212, 16: P016 / P216 (= NV12 / NV16 at 16 bits).
 * *num_comps = 3, *bytes = grk_amd_surface_bytes.  GRK_AMD_ERR_INVALID: an unknown format, a pitch below a row or no multiple of
 * bps, P016 / P216 with prec <= 8; GRK_AMD_ERR_UNSUPPORTED: prec > 16. */
#define GRK_AMD_SURFACE_NV12 0
#define GRK_AMD_SURFACE_NV21 1
#define GRK_AMD_SURFACE_I420 2
#define GRK_AMD_SURFACE_YV12 3
#define GRK_AMD_SURFACE_NV16 4
#define GRK_AMD_SURFACE_I422 5
#define GRK_AMD_SURFACE_I444 6
#define GRK_AMD_SURFACE_P016 7
#define GRK_AMD_SURFACE_P216 8
int grk_amd_surface_format(int format, const grk_amd_image_layout* im, uint32_t prec, uint64_t pitch, grk_amd_surface* surface,
                           uint8_t* comp_dx, uint8_t* comp_dy, uint32_t* num_comps, uint64_t* bytes);
/* host only, no context: the plan of grk_amd_encode_surface (decode = 0) / grk_amd_decode_surface (decode != 0) for a surface of
 * `cap` bytes whose base address is `base_align` modulo 4.  A unit -- a tile's run of consecutive components with equal factors --
 * of a ONE-tile image goes to the tile coder IN PLACE, on the surface's own pointer, where the run is a grk_amd_pixel_layout:
 *   planar       step 1, one pitch, a single component or offsets rising by one plane pitch of at least a plane's span;
 *   interleaved  one step in 2..4 and one pitch of at least w * step * bps, offsets bps apart in component order; an encode takes
 *                step >= the run's components (the others are skipped) where the pixels' extent lies inside `cap`, a decode needs
 *                step == components (it would write `fill` into the others);
 *   alignment    a decode's first sample on a 4-byte address (the inverse transform's pixel stores of the default layout are pairs
 *                and dwords; pitched and interleaved stores fall back to single samples for odd pitches by themselves); an
 *                encode's on a multiple of bps (8-bit device pixels off 4-byte alignment take the separate ingest pass).
 * Every other unit -- multi-tile images, reversed component order (NV21, YV12), a lone component of interleaved pixels on decode,
 * destinations off alignment, and every run with a component of shift != 0 (the two kernels apply the shift; the tile coders and
 * grk_amd_pixel_layout know none) -- is STAGED: cut out of / placed onto the surface by a kernel, through tight planes.  allow_direct = 0:
 * all staged (what GRK_AMD_SURFACE_DIRECT=0 does).  in_place[r] (cap_runs entries, may be NULL): 1 / 0 per run, layouts[r] the layout
 * of an in-place run, at[r] its first sample's offset.  Returns the number of runs, GRK_AMD_ERR_OVERFLOW when grk_amd_surface_bytes
 * exceeds `cap` (or cap_runs is too small), else the surface's refusal; *why as above. */
int grk_amd_surface_plan(const grk_amd_image_layout* im, const grk_amd_tile_params* base, const uint8_t* comp_dx, const uint8_t* comp_dy,
                         const grk_amd_surface* surface, uint64_t cap, uint32_t base_align, int decode, int allow_direct,
                         uint8_t* in_place, grk_amd_pixel_layout* layouts, uint64_t* at, uint32_t cap_runs, const char** why);
/* Surface -> codestream.  `pixels`: the surface's base, host memory or (pixels_on_device != 0) device memory, `cap` bytes.  The file is
 * byte-identical to grk_amd_encode_image_subsampled's for the same samples as tight planes (all factors 1: to grk_amd_encode_image's in
 * the default layout, colour transform included): same flags, any tile layout, image offsets, precincts, the five orders.  Units
 * are coded in place or staged as grk_amd_surface_plan says (GRK_AMD_SURFACE_DIRECT=0, read per call: all staged); a host surface goes
 * up as one copy of its extent.  Tier-2 runs on the device, as for grk_amd_encode_image: every batch's rows and coded bytes stay in
 * device memory, the tile-parts are assembled there and fetched, the main header is written by the host from their lengths
 * (GRK_AMD_IMAGE_T2=host, read per call: the host writer over the fetched rows, which is also where a layout beyond the device
 * writer's tables and GRK_AMD_CS_BLOCK_MSBS go, silently; the file is the same byte for byte -- grk_amd_encode_route_counters
 * tells which ran).  grk_amd_encode_image_subsampled and grk_amd_encode_packed follow the same rule.  The context's pixel layouts
 * are neither consulted nor changed.  GRK_AMD_ERR_OVERFLOW before any work when the surface does not fit `cap`. */
int64_t grk_amd_encode_surface(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                               const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                               const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, uint8_t* out, uint64_t out_cap);
/* The same file left in DEVICE memory: *d_file points at SOC .. EOC, contiguous, in a buffer the context owns, valid until the next
 * encode call of that context; returns its length.  Only the tile-parts' lengths come to the host (the main header's size does not
 * depend on them: the tile-parts are assembled behind room for it, then the header and EOC are uploaded).  There is no host writer
 * behind this call: GRK_AMD_ERR_UNSUPPORTED where the device writer does not reach (GRK_AMD_CS_BLOCK_MSBS, TLM over 255 tiles, tables
 * beyond its fields), GRK_AMD_IMAGE_T2 is not consulted.  Synchronous: complete on return. */
int64_t grk_amd_encode_surface_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                      const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                      const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, void** d_file);
/* cumulative per context, over grk_amd_encode_image_subsampled, grk_amd_encode_surface, grk_amd_encode_packed and the two _device
 * calls: which = 0 files whose tile-parts were assembled on the device, 1 files written by the host writer */
uint64_t grk_amd_encode_route_counters(grk_amd_ctx* ctx, int which);
/* ... in a file of at most rate->target_bytes (rate-targeted encodes, above: always over joint tables).  The same resolution, routes
 * and staging; a unit's pixels are cut out again for a round's final launch when another batch has used the context since; the
 * counters count a unit once per call.  The file equals grk_amd_encode_image_subsampled_rate's for the same samples as tight planes
 * and the same target, in place or staged. */
int64_t grk_amd_encode_surface_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                    const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                    const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, const grk_amd_rate* rate,
                                    uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result);
/* ... for quality->target_psnr (quality-targeted encodes, above): the file equals grk_amd_encode_image_subsampled_quality's for the
 * same samples as tight planes */
int64_t grk_amd_encode_surface_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                       const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                       const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, const grk_amd_quality* quality,
                                       uint8_t* out, uint64_t out_cap, grk_amd_quality_result* result);
/* Codestream -> surface: component c's samples on the surface are plane c of grk_amd_decode_image, every component at its own size
 * (no view, no upsampling: the context's pixel layouts and grk_amd_set_decode_upsample are neither consulted nor changed), and every
 * byte of [pixels, pixels + cap) that is no sample of a component keeps its value (a host surface travels both ways for that).  A
 * device surface is asynchronous behind the reader: grk_amd_decode_status joins and reports, the int16-plane rule included; with a
 * host surface the call repeats such a group with int32 planes by itself.  GRK_AMD_ERR_UNSUPPORTED as grk_amd_decode_image (a context
 * with a decode reduce or a decode sequence among it); GRK_AMD_ERR_OVERFLOW, before anything is written, when the surface does not
 * fit `cap`; GRK_AMD_ERR_INVALID for components that share bytes.  QCD words and segments are put back on return. */
int grk_amd_decode_surface(grk_amd_ctx* ctx, const uint8_t* cs, uint64_t len, const grk_amd_surface* surface,
                           void* pixels, uint64_t cap, int pixels_on_device);
/* cumulative per context: which = 0 units handled in place, 1 units staged, 2 launches of the two surface kernels */
uint64_t grk_amd_surface_counters(grk_amd_ctx* ctx, int which);
/* The two kernels alone (device pointers; queued on the context's stream).  nunits units of ncomp x h x w samples of bps (1 or 2)
 * bytes lie back to back, tight, component-major at `tiles`; unit i's first sample is sample (origins[2 i], origins[2 i + 1]) of
 * each component; comps[k] (ncomp <= 4 of them) places component k on the surface (row_pitch here is taken as it is: not 0).
 * cut: surface -> tiles, word >> comps[k].shift; place: tiles -> surface, v << comps[k].shift cut to the container, writing no byte
 * that is no sample (two partners of step 2 in one call are merged into 16-byte stores); shift < 8 * bps.  Every sample is checked
 * against surface_bytes on the host: GRK_AMD_ERR_INVALID outside it. */
int grk_amd_surface_cut_device(grk_amd_ctx* ctx, const void* surface, uint64_t surface_bytes, const grk_amd_surface_comp* comps, uint32_t ncomp,
                               uint32_t bps, uint32_t nunits, uint32_t w, uint32_t h, const uint32_t* origins, void* tiles);
int grk_amd_surface_place_device(grk_amd_ctx* ctx, const void* tiles, uint32_t nunits, uint32_t w, uint32_t h, uint32_t ncomp, uint32_t bps,
                                 const uint32_t* origins, const grk_amd_surface_comp* comps, void* surface, uint64_t surface_bytes);

/* ---- packed 4:2:2 video frames: YUY2, UYVY, YVYU, Y210 / Y212 / Y216, v210 (packed_format.h, packed.cpp, kernels_packed.hip) ------
 * What a capture card (UYVY, v210) and Direct3D / VA-API (YUY2, Y210, Y216) hand out: ONE pitched frame whose components differ in
 * step -- no grk_amd_surface.  Always three components Y, Cb, Cr with factors (1, 1), (2, 1), (2, 1), no colour transform; sample
 * (0, 0) of the frame is the image area's first luma sample, whose x0 must be even.  For an area of w x h the luma plane is w x h,
 * each chroma plane cw x h with cw = ceil(w / 2); macropixel m of a row holds Y[2m], Y[2m + 1], Cb[m], Cr[m]:
 *   YUY2 / UYVY / YVYU  4 bytes: Y0 Cb Y1 Cr / Cb Y0 Cr Y1 / Y0 Cr Y1 Cb; prec 1..8; any base, pitch 0 = 4 cw
 *   Y216                4 little-endian 16-bit words Y0 Cb Y1 Cr, each v << (16 - prec); prec 9..16 (10: Y210, 12: Y212); base and
 *                       pitch even, pitch 0 = 8 cw
 *   V210                a 16-byte block of four little-endian dwords with 10-bit fields at bits 0-9, 10-19, 20-29 (30-31 zero) holds
 *                       three macropixels -- block b of a row: w0 = Cb[3b] | Y[6b] << 10 | Cr[3b] << 20, w1 = Y[6b+1] | Cb[3b+1] << 10 |
 *                       Y[6b+2] << 20, w2 = Cr[3b+1] | Y[6b+3] << 10 | Cb[3b+2] << 20, w3 = Y[6b+4] | Cr[3b+2] << 10 | Y[6b+5] << 20;
 *                       prec exactly 10; a row is ceil(w / 6) blocks; base and pitch multiples of 16, pitch 0 = ceil(w / 48) * 128
 * An encode ignores the low 16 - prec bits of a Y216 word, bits 30-31 of a v210 dword and every field past the width (Y1 of an odd
 * width's last macropixel, the unused fields of the last v210 block).  A decode writes exactly the bytes of samples (an odd width's
 * last Y1 and everything between a row's end and the pitch keep their values); v210: every block that holds a sample is written
 * whole, fields past the width and bits 30-31 as zero, the bytes behind a row's last block keep their values.
 * One kernel pair moves the frame to and from three tight planes that the context owns (each from a 256-byte boundary, so that a
 * one-tile image's planes take the in-place routes of grk_amd_surface_plan); between them the calls are the surface calls above on
 * that device surface.  The context's pixel layouts, upsample switch and QCD words are neither consulted nor left changed.
 * Refusals, before any GPU work (the reason: *why, or grk_amd_last_error) -- GRK_AMD_ERR_INVALID: an unknown format, a precision
 * outside the format's range, a pitch below a row, a pitch or a device base off the format's alignment, num_comps != 3, mct != 0;
 * GRK_AMD_ERR_UNSUPPORTED: an odd x0, and on decode a stream whose SIZ is not 3 components with factors (1, 1), (2, 1), (2, 1) and a
 * precision of the format; GRK_AMD_ERR_OVERFLOW: grk_amd_packed_bytes > cap.  What the surface and rate calls refuse is passed on. */
#define GRK_AMD_PACKED_YUY2 0
#define GRK_AMD_PACKED_UYVY 1
#define GRK_AMD_PACKED_YVYU 2
#define GRK_AMD_PACKED_Y216 3
#define GRK_AMD_PACKED_V210 4
/* host only: *pitch (0 on entry = the format's default) checked and filled in; returns the bytes from the base to the end of the
 * last row's last container, 0 + *why (may be NULL; a string of the library's) on a refusal */
uint64_t grk_amd_packed_bytes(int format, const grk_amd_image_layout* im, uint32_t prec, uint64_t* pitch, const char** why);
/* Packed frame -> codestream: byte-identical to grk_amd_encode_image_subsampled for the same samples as tight planes with factors
 * (1, 1), (2, 1), (2, 1) and the same flags (any tile layout, precincts, the five orders); base: num_comps 3, mct 0, prec as the
 * format allows.  pixels: host or (pixels_on_device != 0) device memory, `cap` bytes; a host frame goes up as one copy. */
int64_t grk_amd_encode_packed(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format, uint64_t pitch,
                              const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, uint8_t* out, uint64_t out_cap);
/* ... left in device memory, as grk_amd_encode_surface_device leaves it (same rules, same lifetime) */
int64_t grk_amd_encode_packed_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                     uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, void** d_file);
/* ... in a file of at most rate->target_bytes: exactly grk_amd_encode_image_subsampled_rate's file for the same target */
int64_t grk_amd_encode_packed_rate(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format, uint64_t pitch,
                                   const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, const grk_amd_rate* rate,
                                   uint8_t* out, uint64_t out_cap, grk_amd_rate_result* result);
/* ... for quality->target_psnr: exactly grk_amd_encode_surface_quality's file for the same samples */
int64_t grk_amd_encode_packed_quality(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format, uint64_t pitch,
                                      const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags, const grk_amd_quality* quality,
                                      uint8_t* out, uint64_t out_cap, grk_amd_quality_result* result);

/* ---- Rate- and quality-targeted files left in DEVICE memory ----------------------------------------------------------------------------
 * The twins of grk_amd_encode_surface_rate / _quality and grk_amd_encode_packed_rate / _quality: the same arguments with `d_file` in place
 * of `out, out_cap` (*d_file: SOC .. EOC, contiguous, in a buffer the context owns, valid until its next encode call, as
 * grk_amd_encode_surface_device has it), the same refusals (pipelining, max_drop, a target that is not a number), the same budgets and
 * rounds -- the file and every field of the result are the host-memory call's.  Tier-2 runs on the device in every round: the block
 * coder's rows stay where they are, their zero bit-planes are made from the chosen drops on the device and written by the header
 * kernel's general tag tree; only the plain encode's rows (16 bytes per block) and each round's tile-part lengths come to the host.
 * GRK_AMD_IMAGE_T2 is not consulted.  The calls end synchronised; a successful one counts in grk_amd_encode_route_counters(ctx, 0).
 * grk_amd_rate_device_counters(ctx, which) of the latest such call -- 0: its Tier-2 passes on the device (the rounds; 1 for a quality
 * target), 1: bytes of coded blocks it copied to the host (0). */
int64_t grk_amd_encode_surface_rate_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                           const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                           const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                           const grk_amd_rate* rate, void** d_file, grk_amd_rate_result* result);
int64_t grk_amd_encode_surface_quality_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                              const uint8_t* comp_dx, const uint8_t* comp_dy, const grk_amd_surface* surface,
                                              const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                              const grk_amd_quality* quality, void** d_file, grk_amd_quality_result* result);
int64_t grk_amd_encode_packed_rate_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                          uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                          const grk_amd_rate* rate, void** d_file, grk_amd_rate_result* result);
int64_t grk_amd_encode_packed_quality_device(grk_amd_ctx* ctx, const grk_amd_image_layout* im, const grk_amd_tile_params* base, int format,
                                             uint64_t pitch, const void* pixels, uint64_t cap, int pixels_on_device, uint32_t flags,
                                             const grk_amd_quality* quality, void** d_file, grk_amd_quality_result* result);
uint64_t grk_amd_rate_device_counters(grk_amd_ctx* ctx, int which);
/* Codestream -> packed frame: component c of the frame is plane c of grk_amd_decode_image, written by the rules above.  A host
 * frame is uploaded, packed into and downloaded (what is no sample stays); the call is synchronous and repeats a group that leaves
 * the int16 planes by itself, as grk_amd_decode_surface does.  A device frame: the pack kernel is queued on the context's stream
 * behind the decode; grk_amd_decode_status joins and reports, GRK_AMD_ERR_RANGE included. */
int grk_amd_decode_packed(grk_amd_ctx* ctx, const uint8_t* cs, uint64_t len, int format, uint64_t pitch, void* pixels, uint64_t cap,
                          int pixels_on_device);
/* The two kernels alone (device pointers; queued on the context's stream).  planes: Y (w x h), Cb, Cr (cw x h each), tight, back
 * to back, samples of bps = prec <= 8 ? 1 : 2 bytes, LSB-aligned, at any address; pitch 0 = the format's default.  The frame's
 * rules are those above (GRK_AMD_ERR_INVALID); GRK_AMD_ERR_OVERFLOW for a planes_bytes or packed_bytes that is too small. */
int grk_amd_packed_unpack_device(grk_amd_ctx* ctx, int format, uint32_t prec, uint32_t w, uint32_t h, const void* packed, uint64_t pitch,
                                 uint64_t packed_bytes, void* planes, uint64_t planes_bytes);
int grk_amd_packed_pack_device(grk_amd_ctx* ctx, int format, uint32_t prec, uint32_t w, uint32_t h, const void* planes, uint64_t planes_bytes,
                               void* packed, uint64_t pitch, uint64_t packed_bytes);
/* cumulative per context: which = 0 launches of the unpack kernel, 1 of the pack kernel */
uint64_t grk_amd_packed_counters(grk_amd_ctx* ctx, int which);

/* ---- one image over the GPUs of a node (node.cpp) -------------------------------------------------------
 * Replaces the reference's tile-level task pool (codestream/CodeStreamCompress.cpp:535-603: tiles are independent tasks whose
 * tile-parts are written in index order) with one grk_amd_ctx + one host thread per device: tile t is coded on device
 * t mod R, and the coded tile-parts are brought together into ONE codestream, byte-identical to the single-GPU file
 *   - flags without GRK_AMD_NODE_GATHER ("parallel writers"): every worker fetches its own coded bytes over its own PCIe
 *     link and runs Tier-2 for its own tiles; the calling thread writes main header (TLM from the sizes) + tile-parts + EOC;
 *   - flags | GRK_AMD_NODE_GATHER: the workers' coded bytes are copied device to device (hipMemcpyPeer: xGMI between GPUs)
 *     into the frame's writer device -- rotating with the frame number -- which brings them to the host in one piece and
 *     runs Tier-2 for all tiles.
 * `devices` lists the HIP devices to use (NULL / 0: all of the node); an entry may repeat (several contexts on one GPU).
 * `pixels` is the whole image, component-major planar, tight, in host memory (pinned or not).
 * In gather mode a worker whose tiles fall into more than one geometry group rotates four buffer sets, so that a group's bytes
 * travel to the writer while the worker's next groups are coded (an event per group, one wait behind the last); the rotation is
 * switched on by the first such encode and multiplies that worker's device memory for planes, arena and tables by four (several
 * GB for 8K tiles).  Parallel writers, and contexts taken through grk_amd_node_ctx before any gather, keep one set.  The rotation
 * STAYS on afterwards: a context taken through grk_amd_node_ctx after such a gather, and every later encode of that worker (gather or
 * not), works with four sets and with the "results valid until the 4th next call" rule of grk_amd_set_pipelining(ctx, 3); a caller
 * that wants the memory back calls grk_amd_set_pipelining(grk_amd_node_ctx(node, i), 0) between images. */
typedef struct grk_amd_node grk_amd_node;
#define GRK_AMD_NODE_GATHER 0x80000000u
int  grk_amd_device_count(void);
int  grk_amd_node_create(const int* devices, uint32_t num_devices, int verbose, grk_amd_node** out);
void grk_amd_node_destroy(grk_amd_node* node);
uint32_t grk_amd_node_size(const grk_amd_node* node);
grk_amd_ctx* grk_amd_node_ctx(grk_amd_node* node, uint32_t i);
const char* grk_amd_node_last_error(grk_amd_node* node);
int64_t grk_amd_node_encode_image(grk_amd_node* node, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                  const void* pixels, uint32_t flags, uint8_t* out, uint64_t cap);
/* The same with the image resident in the memory of HIP device `pixels_device` (same layout): every worker cuts its tiles out of it
 * with 2-D device-to-device copies -- from another GPU's memory over xGMI, peer access is switched on by grk_amd_node_create --,
 * so that no pixel crosses PCIe (the host-pixels entry is PCIe-bound by construction).  Same codestream, byte for byte. */
int64_t grk_amd_node_encode_image_device(grk_amd_node* node, const grk_amd_image_layout* im, const grk_amd_tile_params* base,
                                         const void* pixels, int pixels_device, uint32_t flags, uint8_t* out, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GROK_AMD_H */
