// Stand-alone check of the model-file parser (babe_amd/csrc/model_file.h), for a host compiler with sanitizers:
//     c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o model_file_check tools/model_file_check.cpp
//     model_file_check [--attention N] FILE...
// Reads each file into a heap buffer of exactly its size (so that a read past the end is a sanitizer report), runs the parser and
// the network validation the loader runs before it touches a device, and prints one line per file: "FILE: ok" or "FILE: refused:
// MESSAGE".  Exit status 0 whatever the verdicts are; non-zero only for a file that cannot be read or a sanitizer report.
// --attention N: validate as babe_model_load_opt does with babe_model_options::attention = N (default 0: attention files refused).
// tests/test_model_file_cpu.py compares the verdicts with babe_model_load's, tests/test_attention_library_cpu.py with
// babe_model_load_opt's.
#include "../babe_amd/csrc/model_file.h"

#include <cstdlib>

int main(int argc, char** argv) {
    int attention = 0, first = 1;
    if (argc > 2 && !strcmp(argv[1], "--attention")) attention = atoi(argv[2]), first = 3;
    for (int i = first; i < argc; ++i) {
        FILE* fh = fopen(argv[i], "rb");
        if (!fh) {
            fprintf(stderr, "%s: cannot open\n", argv[i]);
            return 2;
        }
        fseek(fh, 0, SEEK_END);
        const long size = ftell(fh);
        fseek(fh, 0, SEEK_SET);
        unsigned char* buf = static_cast<unsigned char*>(malloc(size > 0 ? (size_t)size : 1));
        if (size < 0 || !buf || fread(buf, 1, (size_t)size, fh) != (size_t)size) {
            fprintf(stderr, "%s: cannot read\n", argv[i]);
            return 2;
        }
        fclose(fh);
        {
            babe_model::File f;
            babe_model::NetCfg cfg;
            std::string err;
            // the loader's order: an empty buffer is handed over as it is (size 0)
            if (babe_model::parse(size > 0 ? buf : nullptr, (size_t)size, f, err) && babe_model::validate(f, cfg, err, attention)) {
                double sum = 0;                       // touch every byte the table points at
                for (const babe_model::Tensor& t : f.tensors)
                    for (size_t k = 0; k < t.numel; ++k) sum += t.data[k];
                printf("%s: ok (%zu tensors, %zu settings, checksum %.6g)\n", argv[i], f.tensors.size(), f.settings.size(), sum);
            } else {
                printf("%s: refused: %s\n", argv[i], err.c_str());
            }
        }
        free(buf);
    }
    return 0;
}
