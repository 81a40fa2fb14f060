// The GGUF parser and the model loader's header path (Gguf::parse, Model::load, Model::check_types;
// blama_amd/csrc/model.cpp) over Q4_0 / Q5_0 images the loader serves and ones it must refuse, as a
// stand-alone host program for a sanitizer build (scripts/legacy_quant_parse_sanitize.py builds it
// with -fsanitize=address,undefined and writes the images).  No GPU: every load is vocab_only.
//
//   t_legacy_quant_parse ok:MODEL.gguf bad=WORD,WORD:MODEL.gguf ...
// Every "ok" header must load; every "bad" one must be refused with a message holding each WORD
// (the tensor and the type by name); each is also re-read at every truncated length (all but the
// alignment padding at its end must be refused).
#include "engine.h"

#include <cstdio>
#include <fstream>
#include <iterator>

static std::vector<uint8_t> slurp(const char* path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static bool load(const uint8_t* p, size_t n, std::string& msg) {
    try {
        mi::Model model;
        mi_model_params mp{0, 0, 1, 0};   // vocab_only
        model.load(p, n, mp);
        return true;
    } catch (const std::exception& e) {
        msg = e.what();
        return false;
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: t_legacy_quant_parse ok:MODEL.gguf bad=WORD,WORD:MODEL.gguf ...\n");
        return 2;
    }
    int fail = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        const bool want_ok = arg.rfind("ok:", 0) == 0;
        const size_t colon = arg.find(':');
        std::vector<std::string> words;
        if (!want_ok) {
            const std::string w = arg.substr(4, colon - 4);
            for (size_t p = 0; p < w.size();) {
                size_t q = w.find(',', p);
                if (q == std::string::npos) q = w.size();
                words.push_back(w.substr(p, q - p));
                p = q + 1;
            }
        }
        const std::vector<uint8_t> img = slurp(arg.substr(colon + 1).c_str());
        std::string msg;
        const bool ok = load(img.data(), img.size(), msg);
        if (ok != want_ok || (!ok && msg.empty())) {
            ++fail;
            std::printf("FAILED %s: loaded=%d (%s)\n", arg.c_str(), (int)ok, msg.c_str());
        }
        for (const std::string& w : words)
            if (msg.find(w) == std::string::npos) {
                ++fail;
                std::printf("FAILED %s: the message lacks '%s' (%s)\n", arg.c_str(), w.c_str(), msg.c_str());
            }
        // truncations: a fresh exact-size copy each, so that a read past the end is a heap overflow
        int refused = 0, tried = 0, must = 0, must_refused = 0;
        for (size_t n = 0; n < img.size(); ++n) {
            std::vector<uint8_t> cut(img.begin(), img.begin() + (long)n);
            std::string m2;
            const bool r = !load(cut.empty() ? img.data() : cut.data(), cut.size(), m2);
            ++tried;
            refused += r;
            if (n + 32 <= img.size()) {   // (the last bytes are padding to the data section's alignment)
                ++must;
                must_refused += r;
            }
        }
        std::printf("%s: %s; %d of %d truncations refused\n", arg.c_str(), ok ? "loaded" : msg.c_str(), refused, tried);
        if (must_refused != must) {
            ++fail;
            std::printf("FAILED %s: a truncated header loaded\n", arg.c_str());
        }
    }
    std::printf("%s (%d failed)\n", fail ? "FAILED" : "ok", fail);
    return fail ? 1 : 0;
}
