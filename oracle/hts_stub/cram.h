/* TEST INFRASTRUCTURE ONLY. Stand-in for htslib's cram.h, written for this project (nothing is taken from htslib).
 * The reference's dataio/bam_handler.h includes sam.h, hts.h, cram.h and hts_endian.h but, on the path the polisher
 * oracle compiles (summary_generator.cpp, simple_aligner.cpp), only names three htslib types, as pointer members of
 * BAM_handler. Declaring them incomplete is enough; no htslib function is declared, so none can be called. */
#ifndef ORACLE_HTS_STUB_CRAM_H
#define ORACLE_HTS_STUB_CRAM_H
typedef struct htsFile htsFile;
typedef struct hts_idx_t hts_idx_t;
typedef struct bam_hdr_t bam_hdr_t;
#endif
