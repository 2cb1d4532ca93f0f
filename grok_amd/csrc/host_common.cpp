// grok_amd/csrc/host_common.cpp -- two host helpers that the HIP-free sources (t2_reader.cpp, decode_image_plan.cpp) share with the
// rest of the library: resolve_pixel_layout (pixel_layout.h) and parallel_for (image.h).  No HIP, no context.
#include "image.h"
#include "pixel_layout.h"
#include <algorithm>
#include <atomic>
#include <thread>

bool resolve_pixel_layout(const grk_amd_tile_params& p, const grk_amd_pixel_layout* l, uint32_t w, uint32_t h, uint32_t ntiles,
                          PixelLayout& o, const char** why)
{
    static const grk_amd_pixel_layout dflt{};
    if (!l) l = &dflt;
    if (!w) w = p.tile_w;
    if (!h) h = p.tile_h;
    const uint64_t bps = (p.prec + 7u) / 8u, nc = p.num_comps;
    auto bad = [&](const char* m) { *why = m; return false; };
    if (!w || !h || !ntiles || !nc || !bps) return bad("pixel layout: no samples");
    if (((uint64_t)w * h) >> 40) return bad("pixel layout: tile too large");
    for (uint64_t v : {l->row_pitch, l->plane_pitch, l->tile_pitch}) {
        if (v % bps) return bad("pixel layout: a pitch is no multiple of the sample size");
        if (v >> 48) return bad("pixel layout: a pitch is out of range");
    }
    uint64_t ch = 1;
    if (l->interleaved) {
        ch = l->channels ? l->channels : nc;
        if (ch < nc || ch > 4) return bad("pixel layout: channels below num_comps or above 4");
        if (l->plane_pitch) return bad("pixel layout: plane_pitch belongs to the planar layout");
    }
    const uint64_t tight_row = (uint64_t)w * ch * bps;
    o.row = l->row_pitch ? l->row_pitch : tight_row;
    if (o.row < tight_row) return bad("pixel layout: row_pitch is smaller than a row");
    const uint64_t plane_span = (uint64_t)(h - 1) * o.row + tight_row;       // first sample .. end of the last row
    uint64_t tile_span, tight_tile;
    if (l->interleaved) {
        o.xstep = (uint32_t)(ch * bps); o.kstep = bps;
        tile_span = plane_span; tight_tile = (uint64_t)h * o.row;
    } else {
        o.xstep = (uint32_t)bps;
        o.kstep = l->plane_pitch ? l->plane_pitch : (uint64_t)h * o.row;
        if (o.kstep < plane_span) return bad("pixel layout: plane_pitch is smaller than a plane");
        tile_span = (nc - 1) * o.kstep + plane_span; tight_tile = nc * o.kstep;
    }
    o.tile = l->tile_pitch ? l->tile_pitch : tight_tile;
    if (o.tile < tile_span) return bad("pixel layout: tile_pitch is smaller than a tile");
    o.channels = (uint32_t)ch;
    o.fill = l->fill;
    o.bytes = (uint64_t)(ntiles - 1) * o.tile + tile_span;
    // (planar with every pitch the tight one IS the default layout, however it was said)
    o.lay = l->interleaved ? 2u : (o.row == tight_row && o.kstep == (uint64_t)h * tight_row && o.tile == nc * o.kstep ? 0u : 1u);
    return true;
}

int grk_amd::parallel_for(size_t n, uint32_t threads, const std::function<int(size_t)>& fn)
{
    threads = (uint32_t)std::max<size_t>(1, std::min<size_t>(threads, n));
    std::atomic<size_t> next{0};
    std::atomic<int> rc{GRK_AMD_OK};
    auto work = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n || rc.load() != GRK_AMD_OK) return;
            const int r = fn(i);
            if (r != GRK_AMD_OK) { int ok = GRK_AMD_OK; (void)rc.compare_exchange_strong(ok, r); }
        }
    };
    std::vector<std::thread> th;
    for (uint32_t i = 1; i < threads; ++i) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return rc.load();
}
