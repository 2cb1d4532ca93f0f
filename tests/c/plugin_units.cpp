// tests/c/plugin_units.cpp -- a C face on the parts of libgrokj2k_plugin.so that need no GPU (grok_amd/csrc/plugin_internal.h), for
// tests/test_plugin_units.py: built together with the plugin's units, linked against libgrok_amd.so.  Plain arrays in and out, so that
// the test fills and reads them with numpy and states its expectations itself.
#include "../../grok_amd/csrc/plugin_internal.h"
#include <memory>

using namespace plugin;

extern "C" {

// -> 1 / 0 (declined); out = {file_size, guard_bits, qstyle, overrides, number of words}
GRA_EXPORT int pu_read_stream_header(const char* path, uint64_t* out, uint16_t* words, uint32_t cap)
{
    StreamHeader h;
    if (!read_stream_header(path, h)) return 0;
    out[0] = h.file_size; out[1] = h.guard_bits; out[2] = h.qstyle; out[3] = h.overrides ? 1 : 0; out[4] = h.words.size();
    for (size_t i = 0; i < h.words.size() && i < cap; ++i) words[i] = h.words[i];
    return 1;
}

// -> 1 / 0 (refused); dims = {w, h, comps, prec, bytes}; the planar buffer into `out` (cap bytes)
GRA_EXPORT int pu_read_pnm(const char* path, uint32_t* dims, uint8_t* out, uint64_t cap)
{
    HostPixels px;
    if (!read_pnm(path, nullptr, px, dims[0], dims[1], dims[2], dims[3])) return 0;
    dims[4] = (uint32_t)px.size();
    if (px.size() > cap) return 0;
    std::memcpy(out, px.data(), px.size());
    return 1;
}

// make_owner(p, comp_params) walked component -> resolution -> band -> precinct -> block:
//   blocks[i] = {x0, y0, x1, y1, comp, res, orientation, precinct}   (cap_blocks rows)
//   bands[j]  = {comp, res, orientation, numPrecincts, blocks in the band}, steps[j] = its stepsize   (cap_bands rows)
//   counts    = {components, resolutions, bands, precincts, blocks}
// comp_params: nullptr or p->num_comps entries.  -> 1, 0 when make_owner declines, -1 when the arrays are too small
GRA_EXPORT int pu_walk_tree(const grk_amd_tile_params* p, const grk_amd_tile_params* comp_params, uint32_t* blocks, uint64_t cap_blocks,
                            uint32_t* bands, float* steps, uint64_t cap_bands, uint64_t* counts)
{
    std::vector<grk_amd_tile_params> cps;
    if (comp_params) cps.assign(comp_params, comp_params + p->num_comps);
    std::unique_ptr<TileOwner> o(make_owner(*p, comp_params ? &cps : nullptr));
    if (!o) return 0;
    const gra_plugin_tile& t = o->tile;
    uint64_t nres = 0, nbands = 0, nprec = 0, nblk = 0;
    for (size_t c = 0; c < t.numComponents; ++c) {
        const gra_plugin_tile_component* tc = t.tileComponents[c];
        for (size_t r = 0; r < tc->numResolutions; ++r, ++nres) {
            const gra_plugin_resolution* res = tc->resolutions[r];
            if (res->level != r) return -1;
            for (size_t b = 0; b < res->numBands; ++b, ++nbands) {
                const gra_plugin_band* band = res->band[b];
                if (nbands >= cap_bands) return -1;
                uint32_t in_band = 0;
                for (uint64_t q = 0; q < band->numPrecincts; ++q, ++nprec)
                    for (uint64_t k = 0; k < band->precincts[q]->numBlocks; ++k, ++nblk, ++in_band) {
                        if (nblk >= cap_blocks) return -1;
                        const gra_plugin_code_block* cb = band->precincts[q]->blocks[k];
                        const uint32_t row[8] = {cb->x0, cb->y0, cb->x1, cb->y1, (uint32_t)c, (uint32_t)r, band->orientation, (uint32_t)q};
                        std::memcpy(blocks + 8 * nblk, row, sizeof row);
                    }
                const uint32_t row[5] = {(uint32_t)c, (uint32_t)r, band->orientation, (uint32_t)band->numPrecincts, in_band};
                std::memcpy(bands + 5 * nbands, row, sizeof row);
                steps[nbands] = band->stepsize;
            }
        }
    }
    counts[0] = t.numComponents; counts[1] = nres; counts[2] = nbands; counts[3] = nprec; counts[4] = nblk;
    return 1;
}

// tile_params_from_header on a header and an image filled from plain numbers:
//   hdr   = {cblockw_init, cblockh_init, irreversible, mct, numresolutions, csty, cblk_sty, t_grid_width, t_grid_height}
//   prcw / prch [33];  bounds = image {x0, y0, x1, y1};  comps[k] = {dx, dy, w, h, x0, y0, prec, sgnd}
// -> 1 / 0 (declined); *tp, *alike, cps[4], cdx[4], cdy[4] as the function left them
GRA_EXPORT int pu_tile_params_from_header(const uint32_t* hdr, const uint32_t* prcw, const uint32_t* prch, const uint32_t* bounds,
                                          uint32_t ncomps, const uint32_t* comps, uint32_t reduce, grk_amd_tile_params* tp, int* alike,
                                          grk_amd_tile_params* cps, uint8_t* cdx, uint8_t* cdy)
{
    gra_header_info h;
    std::memset(&h, 0, sizeof h);
    h.cblockw_init = hdr[0]; h.cblockh_init = hdr[1]; h.irreversible = hdr[2] != 0; h.mct = hdr[3]; h.numresolutions = hdr[4];
    h.csty = (uint8_t)hdr[5]; h.cblk_sty = (uint8_t)hdr[6]; h.t_grid_width = hdr[7]; h.t_grid_height = hdr[8];
    for (int r = 0; r < GRA_J2K_MAXRLVLS; ++r) { h.prcw_init[r] = prcw[r]; h.prch_init[r] = prch[r]; }
    std::vector<gra_image_comp> cs(ncomps);
    for (uint32_t k = 0; k < ncomps; ++k) {
        const uint32_t* v = comps + 8 * k;
        std::memset(&cs[k], 0, sizeof cs[k]);
        cs[k].dx = v[0]; cs[k].dy = v[1]; cs[k].w = v[2]; cs[k].h = v[3]; cs[k].x0 = v[4]; cs[k].y0 = v[5];
        cs[k].prec = (uint8_t)v[6]; cs[k].sgnd = v[7] != 0;
    }
    gra_image img;
    std::memset(&img, 0, sizeof img);
    img.x0 = bounds[0]; img.y0 = bounds[1]; img.x1 = bounds[2]; img.y1 = bounds[3];
    img.numcomps = (uint16_t)ncomps; img.comps = cs.data();
    HeaderTile t;
    if (!tile_params_from_header(h, &img, reduce, t)) return 0;
    *tp = t.tp; *alike = t.alike ? 1 : 0;
    for (size_t c = 0; c < t.cps.size() && c < 4; ++c) cps[c] = t.cps[c];
    std::memcpy(cdx, t.cdx, 4); std::memcpy(cdy, t.cdy, 4);
    return 1;
}

// params_from_cparameters on a gra_cparameters filled from plain numbers (everything else zero, roi_compno = -1 when cfg says so):
//   cfg = {isHT, cblk_sty, tile_size_on, tx0, ty0, t_width, t_height, numpocs, roi_compno + 1, subsampling_dx, subsampling_dy,
//          image_offset_x0, image_offset_y0, numresolution, irreversible, tcp_mct, cblockw_init, cblockh_init, csty, res_spec,
//          tcp_numlayers};  prcw / prch [33];  img = {w, h, comps, prec, multi}
GRA_EXPORT int pu_params_from_cparameters(const uint32_t* cfg, const uint32_t* prcw, const uint32_t* prch, const uint32_t* img,
                                          grk_amd_tile_params* p)
{
    auto cp = std::make_unique<gra_cparameters>();
    std::memset(cp.get(), 0, sizeof(gra_cparameters));
    cp->isHT = cfg[0] != 0; cp->cblk_sty = (uint8_t)cfg[1]; cp->tile_size_on = cfg[2] != 0;
    cp->tx0 = cfg[3]; cp->ty0 = cfg[4]; cp->t_width = cfg[5]; cp->t_height = cfg[6];
    cp->numpocs = cfg[7]; cp->roi_compno = (int32_t)cfg[8] - 1;
    cp->subsampling_dx = cfg[9]; cp->subsampling_dy = cfg[10]; cp->image_offset_x0 = cfg[11]; cp->image_offset_y0 = cfg[12];
    cp->numresolution = (uint8_t)cfg[13]; cp->irreversible = cfg[14] != 0; cp->tcp_mct = (uint8_t)cfg[15];
    cp->cblockw_init = cfg[16]; cp->cblockh_init = cfg[17]; cp->csty = (uint8_t)cfg[18]; cp->res_spec = cfg[19];
    cp->tcp_numlayers = (uint16_t)cfg[20];
    for (int r = 0; r < GRA_J2K_MAXRLVLS; ++r) { cp->prcw_init[r] = prcw[r]; cp->prch_init[r] = prch[r]; }
    return params_from_cparameters(cp.get(), img[0], img[1], img[2], img[3], *p, img[4] != 0) ? 1 : 0;
}

} // extern "C"
