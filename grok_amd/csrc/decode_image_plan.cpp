// grok_amd/csrc/decode_image_plan.cpp -- the host planning of the whole-image decodes (decode_image_plan.h).  No HIP, no context:
// every route, refusal, offset and size that decode_image.cpp acts on is decided here, where a CPU test reaches it
// (tests/test_decode_image_plan_cpu.py).
#include "decode_image_plan.h"
#include <algorithm>

namespace grk_amd {
namespace {
int refuse(const char** why, int rc, const char* text) { *why = text; return rc; }

// the Staged route: every geometry group one batch into staging, KP or KU behind it
void plan_staged(const grk_amd_stream_info& info, const ViewPlan& plan, const ImageDestIn& in, ImageDest& d)
{
    const uint32_t nc = info.base.num_comps, bps = d.bps;
    const PixelLayout& ipx = d.ipx;
    d.upload_image = (!d.sub || d.up) && ipx.lay;
    // the tile decoder writes tight tiles in the same kind of layout; KP places them by rows of whole pixels and clips them to the
    // view.  Runs of sub-sampled components are decoded as tight planes: KP places them in the components' planes, KU on the reference grid
    const bool whole_pixels = !d.sub && ipx.lay == 2;
    d.unit_ch = whole_pixels ? ipx.channels : 0;
    if (whole_pixels) { d.tile_layout.interleaved = 1; d.tile_layout.channels = (uint8_t)ipx.channels; d.tile_layout.fill = in.layout.fill; }
    d.kstep = ipx.lay == 2 ? bps : ipx.kstep;
    for (const auto& G : d.g.members) {
        // group after group: where a unit goes in its components' planes of the view (signed: KP clips) -- or, for KU, its first
        // sample in the component
        ImageGroup grp{};
        grp.p = d.tp[G[0]];
        grp.units = G;
        grp.uw = plan.units[G[0]].w; grp.uh = plan.units[G[0]].h;          // (the group's units at the view's reduce)
        grp.skip = !grp.uw || !grp.uh;
        grp.unit_size = (uint64_t)grp.uw * grp.uh * (d.unit_ch ? d.unit_ch : grp.p.num_comps) * bps;
        grp.place_at = d.places.size() / 2;
        for (uint32_t u : G) {
            d.places.push_back(d.up ? d.tp[u].tile_x0 : (uint32_t)plan.units[u].x);
            d.places.push_back(d.up ? d.tp[u].tile_y0 : (uint32_t)plan.units[u].y);
        }
        d.group_bytes = std::max<uint64_t>(d.group_bytes, grp.unit_size * G.size());
        for (const RunSegment& s : run_segments(G, d.nr)) {      // the group's units of one run: one launch into that run's planes
            const CompRun& run = plan.runs[s.run];
            ImageLaunch l{};
            l.seg = s;
            if (d.up) {
                l.at = run.first * d.kstep; l.ncomp = run.count; l.bps = bps; l.w = (uint32_t)d.W; l.h = (uint32_t)d.H;
                l.row = ipx.row; l.kstep = d.kstep; l.dx = info.comp_dx[run.first]; l.dy = info.comp_dy[run.first];
            } else if (d.sub) {
                const ImagePlane& pl = d.plane[run.first];
                l.at = pl.at; l.ncomp = run.count; l.bps = bps; l.w = (uint32_t)pl.w; l.h = (uint32_t)pl.h;
            } else {
                // (interleaved pixels are placed as one component of samples as wide as a pixel)
                l.ncomp = ipx.lay == 2 ? 1u : nc; l.bps = ipx.lay == 2 ? d.unit_ch * bps : bps; l.w = (uint32_t)d.W; l.h = (uint32_t)d.H;
                l.row = ipx.lay ? ipx.row : 0; l.kstep = ipx.lay == 1 ? ipx.kstep : 0;
            }
            grp.launches.push_back(l);
        }
        d.groups.push_back(std::move(grp));
    }
    d.places_room = d.places.size() * 4;
    if (!d.up) return;
    // what no footprint covers: the strip left of and above a component's first sample (image origins that are no multiple of
    // the factor) is 0, the samples beyond num_comps of interleaved pixels are `fill`
    const uint32_t W = (uint32_t)d.W, H = (uint32_t)d.H;
    for (uint32_t k = 0; k < nc; ++k) {
        const uint32_t zx = (uint32_t)std::min<uint64_t>(d.W, d.plane[k].x0 * info.comp_dx[k] - info.layout.x0);
        const uint32_t zy = (uint32_t)std::min<uint64_t>(d.H, d.plane[k].y0 * info.comp_dy[k] - info.layout.y0);
        d.fills.push_back(FillRect{k, 0, 0, zx, H, 0});
        d.fills.push_back(FillRect{k, zx, 0, W - zx, zy, 0});
    }
    for (uint32_t k = nc; ipx.lay == 2 && k < ipx.channels; ++k) d.fills.push_back(FillRect{k, 0, 0, W, H, ipx.fill});
}

// the Surface route: a run of a one-tile image that surface_plan.h finds expressible as a pixel layout is decoded straight onto the
// surface through it, every other unit into tight planes that KD places
void plan_onto_surface(const grk_amd_stream_info& info, const ViewPlan& plan, const ImageDestIn& in, ImageDest& d)
{
    d.surf_route.resize(d.nr);
    for (uint32_t r = 0; r < d.nr; ++r)
        d.surf_route[r] = plan_surface_run(d.rs, plan.runs[r], info.num_tiles == 1, true, in.surface_direct, in.pixels_on_device ? in.cap : d.total, in.dst_align);
    SurfaceStaging st = plan_surface_staging(d.g.members, d.surf_route, d.rs, plan.runs, d.tp);      // (the members: sorted run by run)
    uint64_t origin_at = 0;
    for (size_t k = 0; k < d.g.members.size(); ++k) {
        ImageGroup grp{};
        for (uint32_t u : d.g.members[k]) if (d.surf_route[u % d.nr].in_place) grp.in_place.push_back(u);
        grp.units = std::move(st.staged[k]);
        grp.skip = grp.units.empty();
        grp.p = d.tp[grp.skip ? d.g.members[k][0] : grp.units[0]];
        grp.uw = grp.p.tile_w; grp.uh = grp.p.tile_h;
        grp.unit_size = (uint64_t)grp.p.tile_w * grp.p.tile_h * grp.p.num_comps * d.bps;
        grp.place_at = origin_at;
        for (const RunSegment& s : st.segments[k]) { ImageLaunch l{}; l.seg = s; grp.launches.push_back(l); }
        origin_at += grp.units.size();
        d.groups.push_back(std::move(grp));
    }
    d.places = std::move(st.origins);
    d.places_room = d.places.size() * 4 + 8;
    d.group_bytes = st.group_bytes;
}
} // namespace

int plan_image_dest(const grk_amd_stream_info& info, const ViewPlan& plan, const ImageDestIn& in, const grk_amd_surface* surf, ImageDest& d,
                    const char** why)
{
    d = ImageDest{};
    *why = "";
    const uint32_t nc = info.base.num_comps, bps = (info.base.prec + 7u) / 8u, nt = info.num_tiles;
    d.bps = bps;
    d.sub = plan.sub || surf; d.up = d.sub && !surf && in.upsample;
    const bool sub = d.sub, up = d.up;
    const uint32_t red = plan.reduce;
    if (red && up) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "a reduced resolution of sub-sampled components together with upsampling (grk_amd_set_decode_upsample)");
    if (sub && !up && !surf) {       // (components of different sizes have no interleaved form, and each plane is tight: as grk_amd_encode_image_subsampled)
        const grk_amd_pixel_layout& l = in.layout;
        if (l.interleaved || l.channels || l.row_pitch || l.plane_pitch || l.tile_pitch)
            return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "a decode pixel layout for sub-sampled components without upsampling (grk_amd_set_decode_upsample)");
    }
    // the units of decoding: a touched tile's runs of components of one size (without sub-sampling: the tile)
    const std::vector<CompRun>& runs = plan.runs;
    if (info.base.mct && !runs[0].mct) return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "the colour transform across components of different size");
    // the view's image (upsampled components: the image area itself; the plan refused every other view of them)
    d.W = up ? (uint64_t)info.layout.x1 - info.layout.x0 : plan.comp_w[0]; d.H = up ? (uint64_t)info.layout.y1 - info.layout.y0 : plan.comp_h[0];
    // ... in the context's decode layout (grk_amd_set_decode_pixel_layout: row_pitch the view's; the default: tight planes) ...
    if (d.W >> 32 || d.H >> 32 || !resolve_pixel_layout(info.base, surf ? nullptr : &in.layout, (uint32_t)d.W, (uint32_t)d.H, 1, d.ipx, why)) return GRK_AMD_ERR_INVALID;
    // ... or, sub-sampled components as they are: component k's plane of its own size, tight, the planes back to back
    d.plane.resize(nc);
    for (uint32_t k = 0; k < nc; ++k) {
        const uint64_t dx = info.comp_dx[k], dy = info.comp_dy[k];
        d.plane[k] = ImagePlane{d.total, plan.comp_w[k], plan.comp_h[k], (info.layout.x0 + dx - 1) / dx, (info.layout.y0 + dy - 1) / dy};
        d.total += d.plane[k].w * d.plane[k].h * bps;
    }
    if (!sub || up) d.total = d.ipx.bytes;
    // ... or wherever the surface puts them: no two of them on one byte, all of it inside `cap`
    if (surf) {
        int rc = resolve_surface(&info.layout, &info.base, info.comp_dx, info.comp_dy, surf, d.rs, why);
        if (!rc) rc = check_surface_disjoint(d.rs, why);
        if (rc) return rc;
        d.total = d.rs.bytes;
    }
    if (d.total > in.cap) return refuse(why, GRK_AMD_ERR_OVERFLOW, "the image does not fit `cap`");
    // the units, grouped by geometry (units of one group are of one size at every reduce: same_geometry compares every resolution)
    const uint32_t nr = (uint32_t)runs.size(), ntt = (uint32_t)plan.tiles.size(), nu = ntt * nr;
    if (!nu) return refuse(why, GRK_AMD_ERR_INVALID, "a view that touches no tile");
    d.nr = nr;
    d.all = ntt == nt;
    d.tp.resize(nu);                  // [touched tile][run]
    for (uint32_t u = 0; u < nu; ++u) {
        d.tp[u] = plan.units[u].p;
        const int rc = add_unit(d.g, d.tp[u]);
        if (rc) return refuse(why, rc, "a tile's geometry");
    }
    // (runs of one geometry -- luma and alpha -- share a group and its batch; they go to different planes: a group's units run by run)
    for (auto& G : d.g.members) std::stable_sort(G.begin(), G.end(), [nr](uint32_t a, uint32_t b) { return a % nr < b % nr; });
    d.ht = !info.base.reserved[0];
    if (d.ht) {
        // HT blocks are decoded against the band's Kmax of the library's own geometry (ensure_geom), not against the stream's QCD
        for (const TileGeom& tg : d.g.geoms)
            for (uint32_t r = 0; r <= info.base.num_levels; ++r)
                for (uint32_t bi = 0; bi < tg.res[r].num_bands; ++bi) {
                    const uint32_t q = r ? 3 * (r - 1) + 1 + bi : 0;
                    const uint32_t expn = info.qstyle ? info.qcd_words[q] >> 11 : info.qcd_words[q] >> 3;
                    if (expn + info.guard_bits - 1u != tg.res[r].band[bi].kmax)
                        return refuse(why, GRK_AMD_ERR_UNSUPPORTED, "an HT stream whose QCD exponents are not the ones this library derives for the geometry");
                }
    }
    // Part-1 blocks of several codeword segments need the segment list; one segment per block is what the table row says
    // -- and so do HT blocks with refinement passes, which only the packets show (in.ht_refine)
    d.want_segs = d.ht ? in.ht_refine : (info.base.reserved[1] & 0x05) != 0;
    // the region decoder's own conditions (grk_amd_decode_region): a DWT level left, samples of at most 16 bits -- and no HT
    // refinement segments, which do not add up to the rows it empties
    const bool region_ok = info.base.num_levels > red && bps <= 2 && !(d.ht && in.ht_refine);
    if (!surf && nt == 1 && nr == 1 && !up && (plan.units[0].whole || region_ok)) {
        // one tile: decoded straight into the destination -- a window of it by the region decoder, whose cost follows the window
        const ViewUnit& u = plan.units[0];
        d.route = u.whole ? ImageRoute::Direct : ImageRoute::Region;
        d.region[0] = (uint32_t)-u.x; d.region[1] = (uint32_t)-u.y;
        d.region[2] = (uint32_t)(-u.x + (int64_t)d.W); d.region[3] = (uint32_t)(-u.y + (int64_t)d.H);
    } else if (!surf && nt == 1 && nr > 1 && !up) {
        // one tile of several runs: run by run straight into the run's planes.  (A plane behind planes of odd size may start off
        // the 4-byte alignment the decoder's pixel stores are written for: such a run in device memory is decoded beside it and copied)
        d.route = ImageRoute::Runs;
        for (uint32_t r = 0; r < nr; ++r) {
            const uint64_t at = d.plane[runs[r].first].at;
            d.run_dest.push_back(RunDest{at, (uint64_t)plan.units[r].w * plan.units[r].h * d.tp[r].num_comps * bps,
                                         in.pixels_on_device && ((in.dst_align + at) & 3u)});
        }
    } else if (surf) {
        d.route = ImageRoute::Surface;
        plan_onto_surface(info, plan, in, d);
    } else {
        d.route = ImageRoute::Staged;
        plan_staged(info, plan, in, d);
    }
    return GRK_AMD_OK;
}

void plan_coded(uint64_t len, uint32_t num_layers, bool all, const std::vector<uint32_t>& tiles, const std::vector<StreamPart>& parts, CodedPlan& o)
{
    const uint32_t ntt = (uint32_t)tiles.size();
    o = CodedPlan{};
    o.part_to.assign(ntt, 0);
    o.span_at.assign(ntt + 1, 0);
    o.up_len = len;
    if (all) o.copies.push_back(CodedCopy{0, 0, len});
    else {
        // tile after tile, a tile's tile-parts in their order (each tile's chain ends within its 255)
        o.up_len = 0;
        for (uint32_t i = 0; i < ntt; ++i) {
            o.part_to[i] = o.up_len;
            for (uint32_t idx = tiles[i], k = 0; k < 255; idx = parts[idx].next, ++k) {
                o.spans.push_back(CodedSpan{parts[idx].at, parts[idx].len, o.up_len});
                o.up_len += parts[idx].len;
                if (!parts[idx].next || parts[idx].next >= parts.size()) break;
            }
            o.span_at[i + 1] = (uint32_t)o.spans.size();
        }
        for (size_t i = 0, j; i < o.spans.size(); i = j) {        // tile-parts that follow each other in the file: one copy
            uint64_t n = o.spans[i].len;
            for (j = i + 1; j < o.spans.size() && o.spans[j].at == o.spans[i].at + n; ++j) n += o.spans[j].len;
            o.copies.push_back(CodedCopy{o.spans[i].to, o.spans[i].at, n});
        }
    }
    // (an appendix holds bytes of what is uploaded: never more than that)
    o.coded_cap = o.up_len + (num_layers > 1 ? o.up_len : 0);
}

int check_moves(const grk_amd_tp_segment* moves, uint64_t n, uint64_t src_bytes, uint64_t dst_bytes, const char** why)
{
    for (uint64_t i = 0; i < n; ++i)
        if (moves[i].src > src_bytes || moves[i].len > src_bytes - moves[i].src || moves[i].dst > dst_bytes || moves[i].len > dst_bytes - moves[i].dst)
            return refuse(why, GRK_AMD_ERR_INVALID, "a move outside its buffers");
    return GRK_AMD_OK;
}

int rebase_table(StreamTable& tab, uint64_t len, bool all, const std::vector<uint32_t>& tiles, const std::vector<StreamPart>& parts, CodedPlan& coded,
                 const ImageDest& dest, std::vector<uint64_t>& unit_row, const char** why)
{
    const uint32_t ntt = (uint32_t)tiles.size(), nr = dest.nr, nu = ntt * nr;
    const uint64_t up_len = coded.up_len;
    if (!all) {
        // the reader's offsets are positions in the codestream (the appendix behind it): onto the compact buffer, each through the
        // tile-part of its tile that it lies in (a tile's tile-parts rise in the file)
        if (coded.span_at.size() != (size_t)ntt + 1) return refuse(why, GRK_AMD_ERR_INVALID, "the coded plan does not fit the tiles");
        for (uint32_t i = 0; i < ntt; ++i) {
            const CodedSpan* const s0 = coded.spans.data() + coded.span_at[i];
            const CodedSpan* const s1 = coded.spans.data() + coded.span_at[i + 1];
            auto onto = [&](uint64_t& at) -> bool {
                const CodedSpan* sp = std::upper_bound(s0, s1, at, [](uint64_t v, const CodedSpan& q) { return v < q.at; });
                if (sp == s0) return false;
                --sp;
                if (at - sp->at > sp->len) return false;
                at = at - sp->at + sp->to;
                return true;
            };
            for (uint64_t k = tab.row_at[i]; k < tab.row_at[i + 1]; ++k) {
                grk_amd_coded_block& row = tab.rows[k];
                if (!row.length) continue;
                if (row.offset >= len) row.offset = row.offset - len + up_len;
                else if (!onto(row.offset)) return refuse(why, GRK_AMD_ERR_INVALID, "a block outside its tile-part");
            }
            for (uint64_t k = tab.move_at[i]; k < tab.move_at[i + 1]; ++k)
                if (!onto(tab.moves[k].src)) return refuse(why, GRK_AMD_ERR_INVALID, "a block outside its tile-part");
        }
    }
    coded.coded_bytes = up_len + tab.appendix_bytes;
    if (coded.coded_bytes > coded.coded_cap) return refuse(why, GRK_AMD_ERR_INVALID, "an appendix larger than the codestream");
    const int rc = check_moves(tab.moves.data(), tab.moves.size(), up_len, tab.appendix_bytes, why);
    if (rc) return rc;
    // a unit's rows in the reader's table: tile after tile, within a tile component after component
    unit_row.assign(nu + 1, 0);
    for (uint32_t u = 0; u < nu; ++u) {
        if (u % nr == 0 && unit_row[u] != tab.row_at[u / nr]) return refuse(why, GRK_AMD_ERR_INVALID, "the reader's table does not fit the tiles");
        unit_row[u + 1] = unit_row[u] + (uint64_t)dest.g.geoms[dest.g.of[u]].blocks_per_comp * dest.tp[u].num_comps;
    }
    if (unit_row[nu] != tab.rows.size()) return refuse(why, GRK_AMD_ERR_INVALID, "the reader's table does not fit the tiles");
    return GRK_AMD_OK;
}

int read_decode_packets(const uint8_t* cs, uint64_t len, const grk_amd_stream_info& info, const std::vector<StreamPart>& parts, const std::vector<uint32_t>* tiles,
                        uint32_t drop_res, uint32_t threads, StreamTable& tab, std::string& err, bool* refined)
{
    *refined = false;
    int rc = read_stream_packets_of(cs, len, info, parts, tiles, drop_res, threads, tab, err);
    if (rc && tab.met_ht_second_pass) {
        *refined = true;
        rc = read_stream_packets_of(cs, len, info, parts, tiles, drop_res, threads, tab, err, true);
    }
    return rc;
}

int replan_for_refinement(const grk_amd_stream_info& info, const ViewPlan& plan, ImageDestIn& in, const grk_amd_surface* surf, const StreamTable& tab, bool refined,
                          ImageDest& d, const char** why)
{
    if (!refined || !d.ht || !table_has_second_segment(tab)) return GRK_AMD_OK;
    in.ht_refine = true;
    return plan_image_dest(info, plan, in, surf, d, why);
}

bool table_has_second_segment(const StreamTable& tab)
{
    for (size_t i = 0; i + 1 < tab.first_segment.size(); ++i) if (tab.first_segment[i + 1] - tab.first_segment[i] > 1) return true;
    return false;
}

bool group_checks_planes16(const ImageDest& d, const grk_amd_tile_params& p) { return d.ht && !d.want_segs && !p.irreversible && p.prec <= 8; }

void group_tables(const StreamTable& tab, const std::vector<uint64_t>& unit_row, const uint32_t* units, size_t n, bool want_segs,
                  std::vector<grk_amd_coded_block>& rows, std::vector<uint32_t>& first, std::vector<grk_amd_segment>& segs)
{
    rows.clear(); first.clear(); segs.clear();
    for (size_t k = 0; k < n; ++k) {
        const uint32_t u = units[k];
        rows.insert(rows.end(), tab.rows.begin() + unit_row[u], tab.rows.begin() + unit_row[u + 1]);
        for (uint64_t i = unit_row[u]; want_segs && i < unit_row[u + 1]; ++i) {
            first.push_back((uint32_t)segs.size());
            segs.insert(segs.end(), tab.segments.begin() + tab.first_segment[i], tab.segments.begin() + tab.first_segment[i + 1]);
        }
    }
    if (want_segs) first.push_back((uint32_t)segs.size());
}

} // namespace grk_amd
