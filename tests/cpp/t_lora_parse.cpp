// The adapter-file parser and validator (Gguf::parse, Lora::load; blama_amd/csrc/model.cpp, lora.cpp)
// over good and malformed images, as a stand-alone host program for a sanitizer build
// (scripts/lora_parse_sanitize.py builds it with -fsanitize=address,undefined and writes the images).
// No GPU: the base model is loaded vocab_only, and the loader uploads nothing.
//
//   t_lora_parse MODEL.gguf (ok|bad):ADAPTER.gguf ...
// Every "ok" file must load, every "bad" one must be refused with a message; each file is also
// re-read at every truncated length of its header region and at a few lengths of its data.
#include "engine.h"

#include <cstdio>
#include <fstream>
#include <iterator>

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::printf("usage: t_lora_parse MODEL.gguf (ok|bad):ADAPTER.gguf ...\n");
        return 2;
    }
    int fail = 0;
    try {
        const std::vector<uint8_t> mimg = slurp(argv[1]);
        mi::Model model;
        mi_model_params mp{0, 0, 1, 0};   // vocab_only
        model.load(mimg.data(), mimg.size(), mp);
        for (int i = 2; i < argc; ++i) {
            const std::string arg = argv[i];
            const bool want_ok = arg.rfind("ok:", 0) == 0;
            const std::string path = arg.substr(arg.find(':') + 1);
            const std::vector<uint8_t> img = slurp(path.c_str());
            bool ok = false;
            std::string msg;
            try {
                auto a = mi::Lora::load(&model, img.data(), img.size());
                ok = a != nullptr;
            } catch (const std::exception& e) {
                msg = e.what();
            }
            if (ok != want_ok || (!ok && msg.empty())) {
                ++fail;
                std::printf("FAILED %s: loaded=%d (%s)\n", arg.c_str(), (int)ok, msg.c_str());
            }
            // truncations: a fresh exact-size copy each, so that a read past the end is a heap overflow
            int refused = 0, tried = 0;
            for (size_t n = 0; n < img.size(); n += (n < 2048 ? 1 : 997)) {
                std::vector<uint8_t> cut(img.begin(), img.begin() + (long)n);
                ++tried;
                try {
                    mi::Lora::load(&model, cut.empty() ? img.data() : cut.data(), cut.size());
                } catch (const std::exception&) {
                    ++refused;
                }
            }
            std::printf("%s: %s; %d of %d truncations refused\n", arg.c_str(), ok ? "loaded" : msg.c_str(), refused, tried);
            if (want_ok && refused != tried) {
                ++fail;
                std::printf("FAILED %s: a truncated image loaded\n", arg.c_str());
            }
        }
    } catch (const std::exception& e) {
        std::printf("FAILED: exception: %s\n", e.what());
        return 1;
    }
    std::printf("%s (%d failed)\n", fail ? "FAILED" : "ok", fail);
    return fail ? 1 : 0;
}
