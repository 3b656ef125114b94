/*
 * cbc_cli.h -- the decode side of the `cbc` command line (cbc_cli_unpack.c), as cbc_main.c calls it.  Every function reads
 * the container `in` and the FASTA `ref`, writes `out` and returns the process's exit status.
 */
#ifndef CBC_CLI_H
#define CBC_CLI_H
#include <stdint.h>

/* --skip-deletions: from here on --depth, --bedcov and --depth-hist count aligned bases only (cbc_gpu_set_depth_skip_deletions on
 * every device they open) with edits_per_read arena entries per read, 1..510; 0: off, the default */
void cbc_cli_skip_deletions(uint32_t edits_per_read);

/* every read, one per line; either file format; contiguous block ranges over the listed devices */
int cbc_cli_decompress(const char *in, const char *out, const char *ref, const int *devs, int ndev);

/* exactly one region (for --sam and --depth: at most one, NULL = the whole file) */
int cbc_cli_decompress_region(const char *in, const char *out, const char *ref, int device, const char *region, int verbose);
int cbc_cli_decompress_sam(const char *in, const char *out, const char *ref, int device, const char *region, int cigar,
                           uint32_t edits_per_read, int verbose);
int cbc_cli_decompress_depth(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude, int verbose);
/* --pileup: at most one region; min_alt >= 1; edits_per_read 1..510, 0 = the library's default; min_alt_ppm 0 (no fraction rule)
 * ..1000000 (--min-alt-frac); by_strand 0 or 1 (--by-strand) */
int cbc_cli_decompress_pileup(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude,
                              uint32_t min_alt, uint32_t edits_per_read, uint32_t min_alt_ppm, int by_strand, int verbose);

/* --consensus: at most one region (NULL: every contig of the table); min_depth >= 1; call_ppm 1..1000000 (--call-frac);
 * line_width 1..65535; flags: CBC_CONS_SHOW_DEL | _FILL_REF | _IUPAC; edits_per_read as for --pileup */
int cbc_cli_decompress_consensus(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude,
                                 uint32_t min_depth, uint32_t call_ppm, uint32_t line_width, uint32_t flags, uint32_t edits_per_read, int verbose);

/* any number of regions and / or a BED file (bed_path NULL: none); output: CBC_TARGETS_READS, _SAM or _DEPTH */
int cbc_cli_decompress_targets(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                               const char *bed_path, uint32_t output, uint32_t exclude, int verbose);
/* n_thr == 0 and !count_reads: the plain summary */
int cbc_cli_decompress_bedcov(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                              const char *bed_path, uint64_t window, uint32_t min_depth, uint32_t exclude, int verbose,
                              const uint32_t *thr, uint32_t n_thr, int count_reads, const uint32_t *pct, uint32_t n_pct);
int cbc_cli_decompress_hist(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                            const char *bed_path, uint32_t max_depth, uint32_t exclude, int verbose);
int cbc_cli_decompress_stats(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                             const char *bed_path, uint32_t exclude, int alignment, uint32_t edits_per_read, int verbose);

#endif
