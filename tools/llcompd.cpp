// llcompd <file.llcomp> [--small-model] [--devices a,b,... | --region x,y,w,h]
//
// Decompressor front end on libllcomp_mi.so with the observable behaviour of the reference tool
// (/root/reference/llcompd.cpp:11-41): one positional argument, the picture is written as "<file>.png", exit status 1
// when the input cannot be read or the stream is rejected with a std::exception (message printed), 2 for any other
// exception, and -- faithfully -- still 0 when only writing the PNG failed (llcompd.cpp:29-31).  stb_image_write is not
// available; tools/image_io.hpp writes the PNG (adaptive row filters, own deflate).  Reads both wire formats.  --small-model: the file is a
// reference-format stream written by a reference built with `LargeModel = false` (llcomp.hpp:21) -- that header does not
// record the variant (a sliced container does).  --devices 0,1,...: a sliced container is decoded over these GPUs inside this
// process (llcomp_mi_decode_devices).  --region x,y,w,h: only that rectangle of the picture is decoded (llcomp_mi_decode_region: only the
// slices of the tiles it touches are read) and written as the PNG; a malformed or out-of-range rectangle, or --region together with
// --devices, is a usage error.
#include <cstdio>
#include <exception>
#include <string>
#include <vector>

#include "../include/llcomp_mi.hpp"
#include "cli_common.hpp"
#include "image_io.hpp"

namespace {

struct Region {
    bool on = false;
    uint32_t x = 0, y = 0, w = 0, h = 0;
};

// "x,y,w,h": four unsigned 32-bit numbers
bool parse_region(const char* text, Region& r) {
    uint64_t v[4];
    const char* p = text;
    for (int i = 0; i < 4; ++i) {
        if (*p < '0' || *p > '9') return false;
        v[i] = 0;
        while (*p >= '0' && *p <= '9') {
            v[i] = v[i] * 10 + uint64_t(*p++ - '0');
            if (v[i] > 0xFFFFFFFFull) return false;
        }
        if (i < 3 && *p++ != ',') return false;
    }
    if (*p) return false;
    r = Region{true, uint32_t(v[0]), uint32_t(v[1]), uint32_t(v[2]), uint32_t(v[3])};
    return true;
}

void usage(const char* argv0) {
    std::fprintf(stderr, "Usage: %s <image_path> [--small-model] [--devices a,b,... | --region x,y,w,h]\n", argv0);
}

int expand_file(const std::string& stream_path, bool legacy_small_model, const std::vector<int>& devices, const Region& region,
                const char* argv0) {
    std::vector<uint8_t> stream;
    if (!cli::slurp(stream_path, stream)) {
        std::fprintf(stderr, "Error opening input file: %s\n", stream_path.c_str());
        return cli::kFailed;
    }
    llcomp_mi_info info;
    uint32_t box[4], covered = 0;
    if (region.on && llcomp_mi_probe(stream.data(), stream.size(), &info) == LLCOMP_MI_OK &&
        llcomp_mi_region_plan(info.width, info.height, info.channels, info.tile_w, info.tile_h, info.planar, region.x, region.y, region.w,
                              region.h, box, &covered) != LLCOMP_MI_OK) {
        usage(argv0);  // a rectangle the picture does not hold (a stream that cannot be probed fails below, as without --region)
        return cli::kFailed;
    }
    llcomp::RawImage picture;
    try {
        picture = region.on ? llcomp::decompressRegion(stream, region.x, region.y, region.w, region.h, -1, legacy_small_model)
                : devices.empty() ? llcomp::decompressImage(stream, -1, legacy_small_model) : llcomp::decompressImage(stream, devices, legacy_small_model);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "Error decompressing image: %s\n", e.what());
        return cli::kFailed;
    } catch (...) {
        std::fprintf(stderr, "Unknown error occurred\n");
        return cli::kUnknown;
    }
    const std::string target = stream_path + ".png";
    const int row_bytes = int(picture.width) * picture.channels;
    if (!image_io::write_png(target, int(picture.width), int(picture.height), picture.channels, picture.pixels.data(), row_bytes))
        std::fprintf(stderr, "Error writing output file: %s\n", target.c_str());  // not an error status in the reference
    return cli::kDone;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        usage(argc ? argv[0] : "llcompd");
        return cli::kFailed;
    }
    bool small = false;
    std::vector<int> devices;
    Region region;
    for (int i = 2; i < argc; ++i) {
        const std::string flag = argv[i];
        if (flag == "--small-model") small = true;
        else if (flag == "--devices" && i + 1 < argc && !cli::parse_device_list(argv[++i], devices)) {
            usage(argv[0]);
            return cli::kFailed;
        } else if (flag == "--region" && (i + 1 >= argc || !parse_region(argv[++i], region))) {
            usage(argv[0]);
            return cli::kFailed;
        }
    }
    if (region.on && !devices.empty()) {  // (region decode over a device list does not exist)
        usage(argv[0]);
        return cli::kFailed;
    }
    return expand_file(argv[1], small, devices, region, argv[0]);
}
