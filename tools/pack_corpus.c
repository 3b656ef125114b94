/* Feeds every NAME.sam / NAME.fa pair of a directory to cbc_pack_sam, serial and with 4 threads, and prints what came back.
 * Meant to be compiled together with the packer under the sanitizers and run on the corpus of tests/packer_corpus.py:
 *
 *   python tests/packer_corpus.py --write-dir /tmp/corpus
 *   gcc -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -o /tmp/pack_corpus \
 *       tools/pack_corpus.c cbc_amd/csrc/cbc_pack.c
 *   /tmp/pack_corpus /tmp/corpus
 *
 * A refused file is an expected outcome (it is printed); the exit status is non-zero only for a file that cannot be read, or
 * when the two thread counts disagree about a file, or when a sanitizer stops the program. */
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../include/cbc_host.h"

static char *slurp(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    char *p = (char *)malloc(n ? (size_t)n : 1);             /* exactly the text: a read past it is the sanitizer's to find */
    if (p && fread(p, 1, (size_t)n, f) != (size_t)n) { free(p); p = NULL; }
    fclose(f);
    *len = (size_t)n;
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
    DIR *d = opendir(argv[1]);
    if (!d) { perror(argv[1]); return 2; }
    int bad = 0, n_files = 0;
    for (struct dirent *e; (e = readdir(d)) != NULL; ) {
        const size_t nl = strlen(e->d_name);
        if (nl < 5 || strcmp(e->d_name + nl - 4, ".sam") != 0) continue;
        char sp[4096], fp[4096];
        snprintf(sp, sizeof sp, "%s/%s", argv[1], e->d_name);
        snprintf(fp, sizeof fp, "%s/%.*s.fa", argv[1], (int)(nl - 4), e->d_name);
        size_t sl = 0, fl = 0;
        char *sam = slurp(sp, &sl), *fa = slurp(fp, &fl);
        if (!sam || !fa) { fprintf(stderr, "cannot read %s or %s\n", sp, fp); return 2; }
        int rc1 = 0; uint64_t recs1 = 0;
        for (uint32_t threads = 1; threads <= 4; threads += 3) {
            cbc_pack_opts o; cbc_pack_default_opts(&o);
            o.block_reads = 16; o.n_threads = threads;
            cbc_packed *p = NULL; char err[512] = "";
            const int rc = cbc_pack_sam(sam, sl, fa, fl, &o, &p, err, sizeof err);
            const uint64_t recs = p ? p->n_recs : 0;
            printf("%-36s threads %u  rc %d  recs %llu  %s\n", e->d_name, threads, rc, (unsigned long long)recs, err);
            if (threads == 1) { rc1 = rc; recs1 = recs; }
            else if (rc != rc1 || recs != recs1) { printf("  ^ differs from the serial path\n"); bad = 1; }
            cbc_packed_free(p);
        }
        free(sam); free(fa); n_files++;
    }
    closedir(d);
    printf("%d files\n", n_files);
    return bad || n_files == 0;
}
