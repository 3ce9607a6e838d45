/*
 * ref_driver_polish.cpp — TEST INFRASTRUCTURE. Builds the REFERENCE's own polisher image builder
 * (SummaryGenerator, pepper/modules/src/pileup_summary/summary_generator.cpp) and read realigner (ReadAligner,
 * pepper/modules/src/local_reassembly/simple_aligner.cpp, which itself includes ssw_cpp.cpp and ssw.c), from the
 * sources where they lie under /root/reference (nothing is copied into this repository), into
 * oracle/_ref/libref_polish.so behind flat C entry points over pv_batch_in.
 *
 * Only compiled where /root/reference exists (this container). Both headers include dataio/bam_handler.h, which
 * includes four htslib headers; oracle/hts_stub/ stands in for them (the three htslib type names BAM_handler's
 * pointer members need). No BAM_handler member is used here, so nothing of htslib is ever linked or called.
 */
#include <cstdint>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "/root/reference/pepper/modules/src/pileup_summary/summary_generator.cpp"
#include "/root/reference/pepper/modules/src/local_reassembly/simple_aligner.cpp"

#include "../include/pepper_hip.h"

static type_read make_read(const pv_batch_in* in, int64_t r) {
    type_read rd;
    rd.pos = in->read_pos[r];
    rd.pos_end = in->read_pos[r];
    rd.flags.is_reverse = (in->read_flags[r] & 1) != 0;
    rd.mapping_quality = in->read_mapq[r];
    rd.read_id = (int)r;
    rd.hp_tag = 0;
    const int64_t b0 = in->base_off[r], b1 = in->base_off[r + 1];
    rd.sequence.assign((const char*)in->bases + b0, (size_t)(b1 - b0));
    if (in->quals) rd.base_qualities.assign(in->quals + b0, in->quals + b1);
    for (int64_t c = in->cigar_off[r]; c < in->cigar_off[r + 1]; c++)
        rd.cigar_tuples.push_back(CigarOp((int)(in->cigar[c] & 0xF), (int)(in->cigar[c] >> 4)));
    return rd;
}

/* Per region g: SummaryGenerator(ref, "contig", ref_start, ref_end).generate_summary(reads, ref_start, ref_end), as
 * AlignmentSummarizer.create_summary calls it. image rows [n][10], genomic_pos (first, second) and row_off
 * [n_regions+1] are written for the first `cap` rows; returns the number of rows of the whole batch. */
extern "C" int64_t ref_polish_flat(const pv_batch_in* in, uint8_t* img, int64_t* pos, int32_t* idx, int64_t* row_off,
                                   int64_t cap) {
    int64_t rows = 0;
    for (int g = 0; g < in->n_regions; g++) {
        row_off[g] = rows;
        std::string ref((const char*)in->ref + in->ref_off[g], (size_t)(in->ref_off[g + 1] - in->ref_off[g]));
        std::vector<type_read> reads;
        for (int64_t r = in->read_off[g]; r < in->read_off[g + 1]; r++) reads.push_back(make_read(in, r));
        SummaryGenerator sg(ref, "contig", in->ref_start[g], in->ref_end[g]);
        sg.generate_summary(reads, in->ref_start[g], in->ref_end[g]);
        for (size_t k = 0; k < sg.image.size(); k++, rows++) {
            if (rows >= cap) continue;
            for (int j = 0; j < 10; j++) img[rows * 10 + j] = sg.image[k][j];
            pos[rows] = sg.genomic_pos[k].first;
            idx[rows] = sg.genomic_pos[k].second;
        }
    }
    row_off[in->n_regions] = rows;
    return rows;
}

/* Per region g: ReadAligner(ref_start, ref_end + 20, window).align_reads_to_reference(reads), as
 * AlignmentSummarizer.reads_to_reference_realignment calls it. window g = win[win_off[g] .. win_off[g+1]).
 * Per input read: state 2 = dropped (not in the output), 1 = kept; new_pos, new_end (type_read::pos, pos_end; the input
 * read's pos_end is its pos) and the output cigar (BAM packing, CigarOp operation in the low 4 bits).
 * Reads for which the reference's behaviour is undefined are not handed to it and get state 3: an empty query, or a
 * read starting at or past the window's end (Align_cpp returns before it clears the Alignment, whose sw_score is then
 * read uninitialised; past the end, substr throws). Outputs are matched to inputs in order: the loop keeps its input
 * order and only skips reads. Returns the cigar words of all reads (written up to cig_cap), or -1 on a mismatch. */
extern "C" int64_t ref_polish_realign(const pv_batch_in* in, const int64_t* win_off, const uint8_t* win, uint8_t* state,
                                      int64_t* new_pos, int64_t* new_end, int64_t* cig_off, uint32_t* cig, int64_t cig_cap) {
    int64_t words = 0;
    std::streambuf* err = std::cerr.rdbuf(nullptr);   /* the loop reports every dropped read on stderr */
    for (int g = 0; g < in->n_regions; g++) {
        const int64_t start = in->ref_start[g], wlen = win_off[g + 1] - win_off[g];
        std::string window((const char*)win + win_off[g], (size_t)wlen);
        std::vector<type_read> reads;
        for (int64_t r = in->read_off[g]; r < in->read_off[g + 1]; r++) {
            const bool undefined = in->read_pos[r] >= start &&
                                   (in->read_pos[r] - start >= wlen || in->base_off[r + 1] == in->base_off[r]);
            state[r] = undefined ? 3 : in->read_pos[r] < start ? 2 : 1;
            if (!undefined) reads.push_back(make_read(in, r));
        }
        ReadAligner aligner((int)start, (int)(in->ref_end[g] + 20), window);
        std::vector<type_read> out = aligner.align_reads_to_reference(reads);
        size_t k = 0;
        for (int64_t r = in->read_off[g]; r < in->read_off[g + 1]; r++) {
            cig_off[r] = words;
            if (state[r] != 1) {
                new_pos[r] = new_end[r] = in->read_pos[r];
                continue;
            }
            if (k >= out.size()) { std::cerr.rdbuf(err); return -1; }
            const type_read& o = out[k++];
            new_pos[r] = o.pos;
            new_end[r] = o.pos_end;
            for (const CigarOp& op : o.cigar_tuples) {
                if (words < cig_cap) cig[words] = ((uint32_t)op.length << 4) | ((uint32_t)op.operation & 0xF);
                words++;
            }
        }
        if (k != out.size()) { std::cerr.rdbuf(err); return -1; }
    }
    const int64_t n_reads = in->n_regions ? in->read_off[in->n_regions] : 0;
    cig_off[n_reads] = words;
    std::cerr.rdbuf(err);
    return words;
}
