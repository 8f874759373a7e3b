// Memory-safety check of the host JPEG stage (csrc/jpeg_host.cpp), a program of its own: build both with the host compiler under
// -fsanitize=address,undefined and run it over a directory of files -- valid ones, truncations, corruptions.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_entropy_check.cpp \
//       diffusionvid_amd/csrc/jpeg_host.cpp -o jpeg_entropy_check && ./jpeg_entropy_check DIR
//
// Every file is copied into a heap block of exactly its size (so that one byte past the end is a sanitizer report), parsed and decoded
// into a buffer of exactly coef_count elements.  Files named ok_* must decode; every other outcome of a call is legal as long as it is a
// return code.  Exit 0 when every file was processed and every ok_* file decoded; the sanitizers abort the program on a finding.
#include <dirent.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/dvid_hip.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    DIR* dir = opendir(argv[1]);
    if (!dir) {
        perror(argv[1]);
        return 2;
    }
    std::vector<std::string> names;
    while (dirent* ent = readdir(dir))
        if (ent->d_name[0] != '.') names.push_back(ent->d_name);
    closedir(dir);
    long n_ok = 0, n_err = 0, n_unsupported = 0, failed = 0;
    for (const std::string& name : names) {
        const std::string path = std::string(argv[1]) + "/" + name;
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) {
            perror(path.c_str());
            return 2;
        }
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = static_cast<uint8_t*>(malloc(size > 0 ? (size_t)size : 1));          // exactly the file: no slack behind it
        if (size > 0 && fread(data, 1, (size_t)size, f) != (size_t)size) {
            perror(path.c_str());
            return 2;
        }
        fclose(f);
        char err[256];
        dvid_jpeg_info info;
        int rc = dvid_jpeg_parse(data, size, &info, err, (int)sizeof(err));
        if (rc == DVID_OK) {
            int16_t* coef = static_cast<int16_t*>(malloc((size_t)info.coef_count * sizeof(int16_t)));
            dvid_jpeg_info again;
            rc = dvid_jpeg_entropy_decode(data, size, coef, info.coef_count, &again, err, (int)sizeof(err));
            if (rc == DVID_OK && (again.coef_count != info.coef_count || again.width != info.width || again.height != info.height)) {
                fprintf(stderr, "%s: parse and entropy_decode disagree\n", name.c_str());
                ++failed;
            }
            long long sum = 0;          // read every coefficient: an uninitialised or unwritten tail would show
            if (rc == DVID_OK)
                for (int64_t i = 0; i < info.coef_count; ++i) sum += coef[i];
            if (sum == 0x7fffffffffffffffLL) puts("");
            free(coef);
        }
        if (rc == DVID_OK) {
            ++n_ok;
        } else {
            rc == DVID_ERR_UNSUPPORTED ? ++n_unsupported : ++n_err;
            if (!err[0]) {
                fprintf(stderr, "%s: code %d without a message\n", name.c_str(), rc);
                ++failed;
            }
            if (!strncmp(name.c_str(), "ok_", 3)) {
                fprintf(stderr, "%s: a valid file was refused (%d): %s\n", name.c_str(), rc, err);
                ++failed;
            }
        }
        free(data);
    }
    printf("%zu files: %ld decoded, %ld malformed, %ld unsupported, %ld failures\n", names.size(), n_ok, n_err, n_unsupported, failed);
    return failed ? 1 : 0;
}
