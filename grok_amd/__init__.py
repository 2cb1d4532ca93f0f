"""grok_amd -- MI355X-native JPEG 2000 / HTJ2K tile processor behind Grok's plugin API.

The product is the C-ABI shared library grok_amd/lib/libgrok_amd.so (HIP kernels for gfx950 +
host geometry / Tier-2) and the plugin shim grok_amd/lib/libgrokj2k_plugin.so.  This Python
package is only the ctypes binding used by bench.py and the tests; it never computes anything
itself and raises loudly when the native library is missing.
"""
from .capi import (PixelLayout, pixel_bytes, TileParams, Block, CodedBlock, Context, lib, lib_path, NativeLibraryMissing,
                   tile_layout, reduced_tile_rect, write_codestream, write_tile_part, write_main_header, locate_tile_parts,
                   CS_TLM, CS_PLT, CS_SOP, CS_EPH, CS_PROG, ImageLayout, layout_tiles, same_tile_geometry, same_tile_packets, write_codestream_layout, Node, NODE_GATHER,
                   StreamInfo, ReaderError, read_header, read_packets, read_packets_parts, read_packets_refine, stream_comp_sizes,
                   ImageView, image_view_size, plan_image_view,
                   Surface, SurfaceComp, SurfaceError, SURFACE_FORMATS, SURFACE_FORMATS_MSB, surface_bytes, surface_plan,
                   PACKED_FORMATS, packed_bytes,
                   CS_BLOCK_MSBS, DROP_SKIP, Rate, RateResult, RateAllocResult, RateError, Quality, QualityResult, QualityAllocResult, StageError, t2_max_block_bytes, t2_max_block_msbs,
                   ERR_UNSUPPORTED, ERR_INVALID, READ_DEVICE_FIRST_COPY,
                   CS_TP, TP_R, TP_L, TP_C, WriterError, tile_part_starts, write_tile_parts, write_main_header_parts)

__all__ = ["PixelLayout", "pixel_bytes", "TileParams", "Block", "CodedBlock", "Context", "lib", "lib_path", "NativeLibraryMissing",
           "tile_layout", "reduced_tile_rect", "write_codestream", "write_tile_part", "write_main_header", "locate_tile_parts", "CS_TLM", "CS_PLT", "CS_SOP", "CS_EPH", "CS_PROG",
           "ImageLayout", "layout_tiles", "same_tile_geometry", "same_tile_packets", "write_codestream_layout", "Node", "NODE_GATHER",
           "StreamInfo", "ReaderError", "read_header", "read_packets", "read_packets_parts", "read_packets_refine", "stream_comp_sizes",
           "ImageView", "image_view_size", "plan_image_view",
           "Surface", "SurfaceComp", "SurfaceError", "SURFACE_FORMATS", "SURFACE_FORMATS_MSB", "surface_bytes", "surface_plan",
           "PACKED_FORMATS", "packed_bytes",
           "CS_BLOCK_MSBS", "DROP_SKIP", "Rate", "RateResult", "RateAllocResult", "RateError", "Quality", "QualityResult", "QualityAllocResult", "StageError", "t2_max_block_bytes", "t2_max_block_msbs",
           "ERR_UNSUPPORTED", "ERR_INVALID", "READ_DEVICE_FIRST_COPY",
           "CS_TP", "TP_R", "TP_L", "TP_C", "WriterError", "tile_part_starts", "write_tile_parts", "write_main_header_parts"]
