// grok_amd/csrc/plugin_internal.h -- what the units of libgrokj2k_plugin.so share (plugin.cpp, plugin_tile.cpp, plugin_files.cpp,
// plugin_encode.cpp, plugin_decode.cpp).  Not installed, not included from include/.  Nothing declared here is exported: the
// library's symbols are the extern "C" entry points of include/grk_plugin_abi.h alone.
#ifndef GRK_AMD_PLUGIN_INTERNAL_H
#define GRK_AMD_PLUGIN_INTERNAL_H
#include "../../include/grk_plugin_abi.h"
#include "image.h"
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#define GRA_EXPORT __attribute__((visibility("default")))
#pragma GCC visibility push(hidden)
namespace plugin {

// ---- plugin.cpp: the contexts, their locks, the debug state ---------------------------------------
struct Dev { grk_amd_ctx* ctx = nullptr; std::mutex* mu = nullptr; std::mutex own; };
extern grk_amd_ctx* g_ctx;             // the device Grok named (grk_plugin_init_info.deviceId): the single-file entry points
extern std::mutex g_mu;                // ... and its lock
extern std::vector<std::unique_ptr<Dev>> g_devs;      // every GPU the batch mode may use: g_ctx first
extern uint32_t g_debug_state;         // GRA_PLUGIN_STATE_*, read from the environment at plugin_init

inline uint32_t ceil_log2(uint32_t v) { uint32_t e = 0; while ((1u << e) < v) ++e; return e; }

// ---- plugin_tile.cpp: the grk_plugin_tile tree ----------------------------------------------------
struct TileOwner {
    gra_plugin_tile tile{};
    grk_amd_tile_params params{};
    std::vector<gra_plugin_tile_component> comps;   std::vector<gra_plugin_tile_component*> comp_ptr;
    std::vector<gra_plugin_resolution> ress;        std::vector<gra_plugin_resolution*> res_ptr;
    std::vector<gra_plugin_band> bands;             std::vector<gra_plugin_band*> band_ptr;
    std::vector<gra_plugin_precinct> precs;         std::vector<gra_plugin_precinct*> prec_ptr;
    std::vector<gra_plugin_code_block> blocks;      std::vector<gra_plugin_code_block*> block_ptr;
    std::vector<grk_amd_coded_block> table;
    std::vector<float> band_steps;                   // the bands' step sizes as make_owner set them (a decode lets the host overwrite them)
    bool served_decode = false;                      // the coded buffer was sized for a decode (every block's worst case + the file)
    bool no_cache = false;                           // per-component geometry (sub-sampled components): not the tree its parameters name
    uint8_t* coded = nullptr; size_t coded_cap = 0; bool coded_pinned = false;
    ~TileOwner() { free_coded(); }
    void free_coded();
    // room for n bytes; keep > 0: the buffer's first `keep` bytes move along when it grows
    bool ensure_coded(grk_amd_ctx* ctx, size_t n, size_t keep = 0);
};
// every component's blocks one behind the other (block.comp = the component) and its precincts per resolution.
// comp_params: sub-sampled components -- the rectangle of every component of the tile (comp_tile_params), each with its own
// block layout and precinct counts; nullptr: every component has p's
struct TreeLayout { std::vector<grk_amd_block> blocks; std::vector<std::vector<uint32_t>> nprec; };
bool tree_layout(const grk_amd_tile_params& p, const std::vector<grk_amd_tile_params>* comp_params, TreeLayout& t);
TileOwner* make_owner(const grk_amd_tile_params& p, const std::vector<grk_amd_tile_params>* comp_params = nullptr);
void patch_owner(TileOwner* o);
TileOwner* acquire_owner(const grk_amd_tile_params& p);
void release_owner(TileOwner* o);
void drop_tile_cache();
// the tile p as an image of one tile, and the rectangle of a component sub-sampled by dx, dy in it (num_comps = 1, no MCT)
grk_amd_image_layout tile_as_image(const grk_amd_tile_params& p);
int comp_tile_params(const grk_amd_tile_params& p, uint32_t dx, uint32_t dy, grk_amd_tile_params& out);
// runs of consecutive components with equal sub-sampling factors: the library's one rule (image.h)
using grk_amd::CompRun;
using grk_amd::comp_runs;
// the tree's components [comp0, comp0 + p->num_comps), which all have p's geometry (the whole tree: comp0 = 0), and the tree of an
// image whose components are sub-sampled each in its own way -- decoded at 1 / 2^reduce of their size (0: full size)
int decode_tree_comps(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const gra_plugin_tile* tile, uint32_t comp0,
                      const uint8_t* band_numbps, uint32_t nbands, uint32_t reduce, void* pixels, int pixels_on_device);
int decode_tree_subsampled(grk_amd_ctx* ctx, const grk_amd_tile_params* p, const uint8_t* comp_dx, const uint8_t* comp_dy,
                           const gra_plugin_tile* tile, const uint8_t* band_numbps, uint32_t nbands, uint32_t reduce, void* planes);

// ---- plugin_files.cpp: what the plugin reads from disk itself (no GPU needed) ---------------------------
// pixels of an image the plugin loads itself: pinned when given a context (the upload is then one DMA at the link's rate)
struct HostPixels {
    uint8_t* p = nullptr; size_t n = 0, cap = 0; bool pinned = false;
    HostPixels() = default;
    HostPixels(const HostPixels&) = delete;
    HostPixels& operator=(const HostPixels&) = delete;
    ~HostPixels() { reset(); }
    void reset();
    bool alloc(grk_amd_ctx* ctx, size_t bytes);
    uint8_t* data() const { return p; }
    size_t size() const { return n; }
};
void drop_pinned_pool();
bool read_pnm(const char* path, grk_amd_ctx* ctx, HostPixels& planar, uint32_t& w, uint32_t& h, uint32_t& comps, uint32_t& prec);
struct StreamHeader {
    uint64_t file_size = 0;
    uint32_t guard_bits = 0, qstyle = 0;
    std::vector<uint16_t> words;          // SPqcd values in band order (8-bit expn << 3 for style 0)
    bool overrides = false;               // QCC / COC / RGN / POC in the main header: per-component deviations
};
bool read_stream_header(const char* path, StreamHeader& h);
// the names in dir that end in one of the extensions (".ppm" ...), in the directory's order
std::vector<std::string> list_files(const std::string& dir, std::initializer_list<const char*> extensions);
constexpr std::initializer_list<const char*> kImageExtensions = {".pgm", ".ppm", ".pnm"};
constexpr std::initializer_list<const char*> kStreamExtensions = {".j2k", ".j2c", ".jp2", ".jph", ".jhc"};
const char* out_extension(int32_t cod_format);

// ---- plugin_encode.cpp: gra_cparameters -> tile parameters, the encode protocol ------------------------
bool single_tile(const gra_cparameters* cp, uint32_t w, uint32_t h);
bool wants_rate_control(const gra_cparameters* cp);
bool params_from_cparameters(const gra_cparameters* cp, uint32_t w, uint32_t h, uint32_t comps, uint32_t prec,
                             grk_amd_tile_params& p, bool multi = false);
int32_t encode_file(gra_cparameters* cp, const char* in, const char* out, gra_encode_callback cb);
int32_t batch_encode(const char* input_dir, const char* output_dir, gra_cparameters* cp, gra_encode_callback cb);
void stop_batch_encode();
bool batch_encode_done();

// ---- plugin_decode.cpp: the host's header -> tile parameters, the decode protocol -----------------------
// the callback record of plugin_decompress (plugin/plugin_interface.h:86-130).  C++ on purpose -- it carries two std::string
// members, so it is no C ABI; plugin and host must share one libstdc++.  Its layout is checked against the reference's own
// struct in oracle/ref_harness/abi_check.cpp.
struct DecodeCallbackInfo {
    size_t deviceId = 0;
    gra_init_decompressors_func init_decompressors_func = nullptr;
    std::string inputFile, outputFile;
    int32_t decod_format = 0, cod_format = 0;             // GRK_UNK_FMT: the host takes them from its own parameters
    void* stream = nullptr; void* codec = nullptr;
    void* decompressor_parameters = nullptr;
    gra_header_info header_info;
    gra_image* image = nullptr;
    bool plugin_owns_image = false;
    gra_plugin_tile* tile = nullptr;
    int32_t error_code = 0;
    uint32_t decompress_flags = 0;
    void* user_data = nullptr;
};
typedef int32_t (*DecodeUserCallback)(DecodeCallbackInfo*);
// what the host's main header says about THE tile: its parameters, and for components sub-sampled each in its own way
// (!alike) every component's rectangle (num_comps = 1) and factors
struct HeaderTile {
    grk_amd_tile_params tp{};
    bool alike = true;
    std::vector<grk_amd_tile_params> cps;
    uint8_t cdx[4] = {1, 1, 1, 1}, cdy[4] = {1, 1, 1, 1};
};
bool tile_params_from_header(const gra_header_info& h, const gra_image* img, uint32_t reduce, HeaderTile& t);
bool band_numbps_from_qcd(const StreamHeader& sh, const grk_amd_tile_params& tp, std::vector<uint8_t>& band_numbps);
int32_t decompress_file(void* params, DecodeUserCallback cb, const char* in_path = nullptr, const char* out_path = nullptr);
int32_t init_batch_decompress(const char* input_dir, const char* output_dir, void* params, DecodeUserCallback cb);
int32_t batch_decompress();
void stop_batch_decompress();
bool batch_decompress_done();

} // namespace plugin
#pragma GCC visibility pop
#endif
