// tests/c/decode_image_plan_refine_units.cpp -- what a whole-image decode decides about an HT file with refinement passes, on the CPU
// (tests/test_decode_image_plan_refine_cpu.py builds it with g++ from the library's HIP-free sources and runs it; its own main).
// It calls what decode_view (decode_image.cpp) calls up to the first launch: header, view plan, destination plan, the packets
// (read_decode_packets: the reader every file goes through and, where that met an HT block's second pass, the one that takes
// refinement passes), replan_for_refinement; then every batch's tables (group_tables) through what decode_impl and run_ht_decode
// make of them (decode_takes_planes16, reduce_segments, select_segments, plan_ht_refinement).
//   decode_image_plan_refine_units FILE reduce x0 y0 x1 y1 planes16     (x1 = 0: no window)
// prints "first <code> reread <0|1> second <0|1> route <before> <after> want_segs <before> <after> checks16 <before> <after> h16 <0|1>
//         batches <n> rows <n> refined <n> dropped <n>" or "refused <code> <reason>"
#include "../../grok_amd/csrc/decode_image_plan.h"
#include "../../grok_amd/csrc/decode_plan.h"
#include "../../grok_amd/csrc/geometry.h"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace grk_amd;

int main(int argc, char** argv)
{
    if (argc != 8) { std::printf("usage: decode_image_plan_refine_units FILE reduce x0 y0 x1 y1 planes16\n"); return 2; }
    std::vector<uint8_t> cs;
    {
        std::FILE* fh = std::fopen(argv[1], "rb");
        if (!fh) { std::printf("cannot read %s\n", argv[1]); return 2; }
        uint8_t buf[65536];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, fh)) > 0;) cs.insert(cs.end(), buf, buf + n);
        std::fclose(fh);
    }
    const uint32_t reduce = (uint32_t)std::atoi(argv[2]), wx0 = (uint32_t)std::atoi(argv[3]), wy0 = (uint32_t)std::atoi(argv[4]), wx1 = (uint32_t)std::atoi(argv[5]),
                   wy1 = (uint32_t)std::atoi(argv[6]);
    const bool planes16 = std::atoi(argv[7]) != 0;
    const uint64_t len = cs.size();
    grk_amd_stream_info info;
    std::string err;
    const char* why = "";
    int rc = read_stream_header(cs.data(), len, info, err);
    if (rc) { std::printf("refused %d %s\n", rc, err.c_str()); return 0; }
    grk_amd_image_view view{};
    view.reduce = reduce; view.x0 = wx0; view.y0 = wy0; view.x1 = wx1; view.y1 = wy1;
    ViewPlan plan;
    rc = plan_image_view(info, (reduce || wx1) ? &view : nullptr, plan, &why);
    if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
    ImageDestIn in;
    in.cap = ~0ull;
    ImageDest d;
    rc = plan_image_dest(info, plan, in, nullptr, d, &why);
    if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
    const int route0 = (int)d.route, want0 = d.want_segs, checks0 = group_checks_planes16(d, d.tp[0]);
    std::vector<StreamPart> parts;
    rc = locate_stream_parts(cs.data(), len, info, parts, err);
    if (rc) { std::printf("refused %d %s\n", rc, err.c_str()); return 0; }
    StreamTable tab;
    // (what the plain reader alone says, for the report)
    StreamTable plain;
    std::string plain_err;
    const int first = read_stream_packets_of(cs.data(), len, info, parts, d.all ? nullptr : &plan.tiles, plan.reduce, 2, plain, plain_err);
    bool reread = false;
    rc = read_decode_packets(cs.data(), len, info, parts, d.all ? nullptr : &plan.tiles, plan.reduce, 2, tab, err, &reread);
    if (rc) { std::printf("refused %d %s\n", rc, err.c_str()); return 0; }
    rc = replan_for_refinement(info, plan, in, nullptr, tab, reread, d, &why);
    if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
    const bool second = in.ht_refine;
    CodedPlan coded;
    plan_coded(len, info.num_layers, d.all, plan.tiles, parts, coded);
    std::vector<uint64_t> unit_row;
    rc = rebase_table(tab, len, d.all, plan.tiles, parts, coded, d, unit_row, &why);
    if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
    // the batches: Direct / Region one unit, Staged a group; each through the decode call's own planning
    std::vector<std::vector<uint32_t>> batches;
    if (d.route == ImageRoute::Direct || d.route == ImageRoute::Region) batches.push_back(d.g.members[0]);
    else for (const ImageGroup& G : d.groups) if (!G.skip) batches.push_back(G.units);
    uint64_t rows = 0, refined = 0, dropped = 0;
    bool h16 = false;
    for (const std::vector<uint32_t>& units : batches) {
        std::vector<grk_amd_coded_block> table;
        std::vector<uint32_t> seg_first, red_first;
        std::vector<grk_amd_segment> segs, red_segs;
        group_tables(tab, unit_row, units.data(), units.size(), d.want_segs, table, seg_first, segs);
        const grk_amd_tile_params& p = d.tp[units[0]];
        TileGeom full, g;
        if (build_tile_geom(p, full)) { std::printf("refused -3 geometry\n"); return 0; }
        g = full;
        if (plan.reduce && reduce_tile_geom(full, plan.reduce, g)) { std::printf("refused -3 reduced geometry\n"); return 0; }
        const uint64_t groups = units.size() * p.num_comps, nblocks = groups * g.blocks_per_comp;
        const uint32_t full_per_comp = plan.reduce ? g.full_blocks_per_comp : g.blocks_per_comp;
        if (table.size() != groups * full_per_comp) { std::printf("refused -3 a batch's rows\n"); return 0; }
        // (decode_impl's question with what grk_amd_set_decode_segments would hold; stage_table: a reduced call keeps each component's
        //  first rows)
        h16 = h16 || decode_takes_planes16(planes16, false, g.p.num_levels >= 1, g.p, !seg_first.empty());
        std::vector<grk_amd_coded_block> kept;
        for (uint64_t k = 0; k < groups; ++k) kept.insert(kept.end(), table.begin() + k * full_per_comp, table.begin() + k * full_per_comp + g.blocks_per_comp);
        if (plan.reduce && !seg_first.empty()) {
            rc = reduce_segments(groups, full_per_comp, g.blocks_per_comp, seg_first, segs, red_first, red_segs, &why);
            if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
        }
        SegList sl;
        rc = select_segments(plan.reduce != 0, seg_first, segs, red_first, red_segs, nblocks, &sl, &why);
        if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
        rows += nblocks; dropped += table.size() - nblocks;
        if (sl.nfirst) {
            std::vector<grk_amd_segment> ref(nblocks);
            uint32_t longest = 0;
            rc = plan_ht_refinement(kept.data(), nblocks, sl, ref.data(), &longest, &why);
            if (rc) { std::printf("refused %d %s\n", rc, why); return 0; }
            for (const grk_amd_segment& s : ref) refined += s.length != 0;
        }
    }
    std::printf("first %d reread %d second %d route %d %d want_segs %d %d checks16 %d %d h16 %d batches %zu rows %llu refined %llu dropped %llu\n", first, (int)reread,
                (int)second, route0, (int)d.route, want0, (int)d.want_segs, checks0, (int)group_checks_planes16(d, d.tp[0]), (int)h16, batches.size(),
                (unsigned long long)rows, (unsigned long long)refined, (unsigned long long)dropped);
    return 0;
}
