// grok_amd/csrc/plugin_files.cpp -- what libgrokj2k_plugin.so reads from disk itself: the pixels of a PNM into a (pinned) buffer,
// the main header of a codestream / JP2 file, the files of a batch directory.  Nothing here needs a GPU.
#include "plugin_internal.h"
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <dirent.h>

namespace plugin {

// (the batch reader takes one HostPixels per file: the pinned ones are recycled through a two-slot pool -- hipHostMalloc /
//  hipHostFree per file cost milliseconds each, and the free waits for the device while the device lock is held)
struct PinnedSlot { uint8_t* p = nullptr; size_t cap = 0; };
static std::mutex g_pin_mu;
static PinnedSlot g_pin_pool[2];
void drop_pinned_pool()
{
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto& sl : g_pin_pool) { if (sl.p) grk_amd_host_free(nullptr, sl.p); sl = PinnedSlot{}; }
}

void HostPixels::reset()
{
    if (p && pinned) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        PinnedSlot* sl = !g_pin_pool[0].p ? &g_pin_pool[0] : !g_pin_pool[1].p ? &g_pin_pool[1]
                         : (g_pin_pool[0].cap <= g_pin_pool[1].cap ? &g_pin_pool[0] : &g_pin_pool[1]);
        if (!sl->p) { sl->p = p; sl->cap = cap; p = nullptr; }
        else if (sl->cap < cap) { std::swap(sl->p, p); std::swap(sl->cap, cap); }      // keep the larger, free the smaller below
    }
    if (p) { if (pinned) grk_amd_host_free(nullptr, p); else std::free(p); }
    p = nullptr; n = 0; cap = 0;
}

bool HostPixels::alloc(grk_amd_ctx* ctx, size_t bytes)
{
    reset();
    if (ctx) {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        int best = -1;                                                                 // the smallest kept buffer that fits
        for (int i = 0; i < 2; ++i)
            if (g_pin_pool[i].p && g_pin_pool[i].cap >= bytes && (best < 0 || g_pin_pool[i].cap < g_pin_pool[best].cap)) best = i;
        if (best >= 0) { p = g_pin_pool[best].p; cap = g_pin_pool[best].cap; g_pin_pool[best] = PinnedSlot{}; }
    }
    if (p) { pinned = true; n = bytes; return true; }
    p = ctx ? static_cast<uint8_t*>(grk_amd_host_alloc(ctx, bytes)) : nullptr;
    pinned = p != nullptr;
    if (!p) p = static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1));
    n = p ? bytes : 0; cap = n;
    return p != nullptr;
}

// ---- minimal PNM (P5/P6, binary) reader: enough for plugin_encode's "read params->infile" -----------
bool read_pnm(const char* path, grk_amd_ctx* ctx, HostPixels& planar, uint32_t& w, uint32_t& h, uint32_t& comps, uint32_t& prec)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    auto token = [&](char* buf, size_t n) -> bool {
        int ch;
        for (;;) {
            ch = std::fgetc(f);
            if (ch == '#') { while ((ch = std::fgetc(f)) != EOF && ch != '\n') {} continue; }
            if (ch == EOF) return false;
            if (ch > ' ') break;
        }
        size_t i = 0;
        while (ch != EOF && ch > ' ' && i + 1 < n) { buf[i++] = (char)ch; ch = std::fgetc(f); }
        buf[i] = 0;
        return i > 0;
    };
    char t[32];
    bool ok = token(t, sizeof t) && t[0] == 'P' && (t[1] == '5' || t[1] == '6') && t[2] == 0;
    comps = ok && t[1] == '6' ? 3 : 1;
    unsigned long maxv = 0;
    ok = ok && token(t, sizeof t) && (w = (uint32_t)std::strtoul(t, nullptr, 10)) > 0;
    ok = ok && token(t, sizeof t) && (h = (uint32_t)std::strtoul(t, nullptr, 10)) > 0;
    ok = ok && token(t, sizeof t) && (maxv = std::strtoul(t, nullptr, 10)) > 0 && maxv < 65536;
    if (!ok) { std::fclose(f); return false; }
    prec = 1; while ((1ul << prec) <= maxv) ++prec;
    const size_t bps = prec > 8 ? 2 : 1, n = (size_t)w * h;
    std::vector<uint8_t> raw(n * comps * bps);
    ok = std::fread(raw.data(), 1, raw.size(), f) == raw.size();
    std::fclose(f);
    if (!ok) return false;
    if (!planar.alloc(ctx, raw.size())) return false;
    uint8_t* const dst = planar.data();
    for (uint32_t c = 0; c < comps; ++c)
        for (size_t i = 0; i < n; ++i) {
            if (bps == 1) dst[c * n + i] = raw[i * comps + c];
            else {   // PNM 16-bit is big endian; the tile buffer is host endian
                const uint8_t* s = &raw[(i * comps + c) * 2];
                reinterpret_cast<uint16_t*>(dst)[c * n + i] = (uint16_t)((s[0] << 8) | s[1]);
            }
        }
    return true;
}

// ---- the stream's own main header: QCD (guard bits, exponents) and the file size ---------------------------------
// The host hands a plugin every block's numbps but not the band's (plugin_bridge.cpp:63-76), and the HT decoder needs
// their difference (missing_msbs).  Grok's own HT streams carry the exponents of HTParams.cpp:248-312 with one guard bit
// (D4 included), which is what grk_amd_tile_layout models; another encoder's stream need not.  So the band numbps come
// from the codestream itself: the file `grk_decompress -i` names in parameters->infile.
bool read_stream_header(const char* path, StreamHeader& h)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::vector<uint8_t> b(1u << 20);
    b.resize(std::fread(b.data(), 1, b.size(), f));
    bool ok = std::fseek(f, 0, SEEK_END) == 0;
    const long sz = std::ftell(f);
    std::fclose(f);
    if (!ok || sz <= 0) return false;
    h.file_size = (uint64_t)sz;
    size_t at = 0;
    auto be16 = [&](size_t i) { return (uint32_t)(b[i] << 8 | b[i + 1]); };
    auto be32 = [&](size_t i) { return (uint32_t)b[i] << 24 | (uint32_t)b[i + 1] << 16 | (uint32_t)b[i + 2] << 8 | b[i + 3]; };
    if (b.size() >= 12 && be32(0) == 12 && be32(4) == 0x6A502020u) {          // JP2: walk the boxes to the codestream
        for (;;) {
            if (at + 8 > b.size()) return false;
            uint64_t len = be32(at);
            const uint32_t type = be32(at + 4);
            size_t hdr = 8;
            if (len == 1) { if (at + 16 > b.size()) return false; len = (uint64_t)be32(at + 8) << 32 | be32(at + 12); hdr = 16; }
            if (type == 0x6A703263u) { at += hdr; break; }                    // 'jp2c'
            if (len < hdr) return false;                                      // (0 = to the end of the file: no codestream box follows)
            if (len > b.size() - at) return false;                            // (a length from the file: never past what was read,
            at += (size_t)len;                                                //  never wrapping back -- the lock is held here)
        }
    }
    if (at + 4 > b.size() || be16(at) != 0xFF4F) return false;
    at += 2;
    bool have_qcd = false;
    while (at + 4 <= b.size()) {
        const uint32_t m = be16(at), len = be16(at + 2);
        if (m == 0xFF90 || m == 0xFF93) break;                                // SOT / SOD: end of the main header
        if (m < 0xFF00 || len < 2 || at + 2 + len > b.size()) return false;
        const size_t d = at + 4, n = len - 2;
        if (m == 0xFF5C && n >= 1) {                                          // QCD
            h.guard_bits = b[d] >> 5; h.qstyle = b[d] & 0x1Fu;
            h.words.clear();
            if (h.qstyle == 0) for (size_t i = 1; i < n; ++i) h.words.push_back(b[d + i]);
            else for (size_t i = 1; i + 1 < n; i += 2) h.words.push_back((uint16_t)be16(d + i));
            have_qcd = true;
        } else if (m == 0xFF5D || m == 0xFF53 || m == 0xFF5E || m == 0xFF5F) {
            h.overrides = true;
        }
        at += 2 + len;
    }
    // the first tile-part header as well: a COD / COC / QCD / QCC / RGN / POC there overrides the main header for that tile,
    // and band_numbps (with it every block's missing_msbs) would come out of the wrong exponents
    if (at + 4 <= b.size() && be16(at) == 0xFF90) {
        at += 2 + be16(at + 2);
        while (at + 4 <= b.size()) {
            const uint32_t m = be16(at), len = be16(at + 2);
            if (m == 0xFF93 || m < 0xFF00 || len < 2) break;
            if (m == 0xFF52 || m == 0xFF53 || m == 0xFF5C || m == 0xFF5D || m == 0xFF5E || m == 0xFF5F) h.overrides = true;
            at += 2 + len;
        }
    }
    return have_qcd;
}

std::vector<std::string> list_files(const std::string& dir, std::initializer_list<const char*> extensions)
{
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string name(e->d_name);
            const size_t dot = name.rfind('.');
            if (dot == std::string::npos) continue;
            const std::string ext = name.substr(dot);
            for (const char* x : extensions)
                if (ext == x) { names.push_back(name); break; }
        }
        closedir(d);
    }
    return names;
}

const char* out_extension(int32_t cod_format)
{
    switch (cod_format) {           // GRK_SUPPORTED_FILE_FMT, grok.h:59-72
    case 3: return ".ppm"; case 4: return ".pgx"; case 5: return ".pam"; case 6: return ".bmp"; case 7: return ".tif";
    case 8: return ".raw"; case 9: return ".png"; case 10: return ".rawl"; case 11: return ".jpg";
    default: return ".ppm";
    }
}

} // namespace plugin
